"""INT4 / INT2 rowwise-quantized inference path (n-bit rows).

The CPU implementations in torchrec_amd/quant/embedding_modules.py are the
oracle; the GPU tests check the HIP kernels against them.

Row error bound used throughout (derived, not measured). For a row with
stored fp16 step ``scale_h`` and extremes ``mn``, ``mx``:

    |deq - w| <= scale_h/2 * (1 + 1e-3) + 2^-10 * (|mn| + |mx|) + 1e-7

Interior points are within half a stored step; clamped points exceed that by
at most the fp16 rounding of L*scale and of mn (each <= 2^-11 relative); the
1e-3 and 1e-7 absorb fp32 arithmetic. The same bound covers the INT8
quantiser (codes against the fp32 scale, dequantised with the fp16 one).
"""

import pytest
import torch

from torchrec_amd.inference.modules import quantize_inference_model
from torchrec_amd.modules.embedding_configs import (
    DATA_TYPE_NUM_BITS,
    DataType,
    EmbeddingBagConfig,
    EmbeddingConfig,
    PoolingType,
    data_type_to_dtype,
)
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection, EmbeddingCollection
from torchrec_amd.quant import (
    dequantize_rowwise_nbit,
    nbit_row_stride,
    quantize_rowwise_nbit,
)
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEBC,
    EmbeddingCollection as QuantEC,
    QuantTableBatchedEmbeddingBags,
    int8_row_stride,
    quantize_rowwise_int8,
    unpack_codes_nbit,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

BITS_OF = {DataType.INT8: 8, DataType.INT4: 4, DataType.INT2: 2}


def stored_scale(packed: torch.Tensor, D: int, bits: int) -> torch.Tensor:
    cb = D * bits // 8
    R = packed.shape[0]
    sb = packed[:, cb : cb + 4].contiguous().reshape(R, 2, 2).view(torch.float16).reshape(R, 2)
    return sb[:, 0].float()


def row_bound(w: torch.Tensor, packed: torch.Tensor, bits: int) -> torch.Tensor:
    """Per-row error bound [R] (module docstring)."""
    D = w.shape[1]
    scale_h = stored_scale(packed, D, bits)
    mn = w.min(dim=1).values
    mx = w.max(dim=1).values
    return scale_h / 2 * (1 + 1e-3) + 2.0**-10 * (mn.abs() + mx.abs()) + 1e-7


def roundtrip_inputs(R: int, D: int):
    g = torch.Generator().manual_seed(0)
    return {
        "randn": torch.randn(R, D, generator=g),
        "narrow": 0.01 * torch.randn(R, D, generator=g) + 3,
        "wide": 100 * torch.rand(R, D, generator=g) - 20,
        "constant": torch.full((R, D), 0.37),
    }


# ---------------------------------------------------------------------------
# mixed-precision EBC / EC fixtures shared by the CPU and GPU tests
# ---------------------------------------------------------------------------

MIXED = [  # (name, D, width, features)
    ("t0", 20, DataType.INT8, ["f0"]),
    ("t1", 8, DataType.INT4, ["f1"]),
    ("t2", 16, DataType.INT2, ["f2"]),
    ("t3", 264, DataType.INT4, ["f3", "f4"]),
    ("t4", 128, DataType.INT2, ["f5"]),
]
MIXED_ROWS = 30
MIXED_B = 5


def mixed_float_ebc(pooling=PoolingType.SUM, weighted=False, specs=MIXED, rows=MIXED_ROWS):
    torch.manual_seed(0)
    tables = [
        EmbeddingBagConfig(
            num_embeddings=rows, embedding_dim=D, name=n, feature_names=list(fs), pooling=pooling
        )
        for (n, D, _, fs) in specs
    ]
    return EmbeddingBagCollection(tables=tables, is_weighted=weighted)


def mixed_dtypes(specs=MIXED):
    return {n: dt for (n, _, dt, _) in specs}


def make_kjt(keys, rows, B, weighted=False, seed=3, empty_key=None):
    """Bag lengths 0..4; the first and the last bag are empty."""
    g = torch.Generator().manual_seed(seed)
    F = len(keys)
    lengths = torch.randint(0, 5, (F * B,), generator=g)
    lengths[0] = 0
    lengths[-1] = 0
    if empty_key is not None:
        k = keys.index(empty_key)
        lengths[k * B : (k + 1) * B] = 0
    n = int(lengths.sum())
    values = torch.randint(0, rows, (n,), generator=g)
    weights = (torch.rand(n, generator=g) * 2 - 0.5) if weighted else None
    return KeyedJaggedTensor(keys=keys, values=values, lengths=lengths, weights=weights, stride=B)


def ebc_tolerance(qebc, float_ebc, kjt, mean: bool, weighted: bool) -> torch.Tensor:
    """[B, total_D] tolerance: per bag, sum over its rows of |psw| * row bound
    (divided by the bag length for MEAN). No free constant."""
    tbe = qebc._tbe
    B = kjt.stride()
    offsets = kjt.offsets()
    values = kjt.values()
    psw = kjt.weights().abs() if weighted else torch.ones(values.numel())
    cols = []
    for f, t in enumerate(tbe._feature_table_map):
        name, rows, D = tbe._specs[t]
        w = float_ebc.embedding_bags[name].weight.detach().cpu().float()
        bound = row_bound(w, tbe.packed_table(t).cpu(), tbe._bits[t])
        tol = torch.zeros(B)
        for b in range(B):
            lo, hi = int(offsets[f * B + b]), int(offsets[f * B + b + 1])
            if hi > lo:
                s = (psw[lo:hi] * bound[values[lo:hi]]).sum()
                tol[b] = s / (hi - lo) if mean else s
        cols.append(tol.unsqueeze(1).expand(B, D))
    return torch.cat(cols, dim=1)


SEQ = [("s0", 32, DataType.INT4, ["fa", "fe"]), ("s1", 32, DataType.INT2, ["fb"])]
SEQ_ROWS = 25


def seq_float_ec():
    torch.manual_seed(0)
    tables = [
        EmbeddingConfig(num_embeddings=SEQ_ROWS, embedding_dim=D, name=n, feature_names=list(fs))
        for (n, D, _, fs) in SEQ
    ]
    return EmbeddingCollection(tables=tables)


def seq_kjt():
    # "fe" has no values at all
    return make_kjt(["fa", "fe", "fb"], SEQ_ROWS, 4, empty_key="fe")


def small_dlrm():
    from torchrec_amd.models.dlrm import DLRM

    torch.manual_seed(0)
    tables = [
        EmbeddingBagConfig(num_embeddings=50, embedding_dim=8, name=f"t{i}", feature_names=[f"f{i}"])
        for i in range(2)
    ]
    return DLRM(
        embedding_bag_collection=EmbeddingBagCollection(tables=tables),
        dense_in_features=4,
        dense_arch_layer_sizes=[8, 8],
        over_arch_layer_sizes=[8, 1],
    )


class TestNbitCpu:
    def test_int2_data_type(self):
        assert DATA_TYPE_NUM_BITS[DataType.INT2] == 2
        assert data_type_to_dtype(DataType.INT2) == torch.uint8

    @pytest.mark.parametrize(
        "D,bits,stride",
        [(128, 8, 144), (128, 4, 80), (128, 2, 48), (8, 4, 16), (16, 2, 16), (264, 4, 144)],
    )
    def test_strides(self, D, bits, stride):
        assert nbit_row_stride(D, bits) == stride
        if bits == 8:
            assert stride == int8_row_stride(D)

    @pytest.mark.parametrize("D,dt", [(12, DataType.INT4), (8, DataType.INT2)])
    def test_bad_dims_rejected(self, D, dt):
        bits = BITS_OF[dt]
        with pytest.raises(ValueError):
            nbit_row_stride(D, bits)
        with pytest.raises(ValueError):
            quantize_rowwise_nbit(torch.zeros(2, D), bits)
        with pytest.raises(ValueError):
            QuantTableBatchedEmbeddingBags([("t", 4, D)], weight_dtypes=[dt])
        with pytest.raises(ValueError):
            QuantEBC(
                tables=[
                    EmbeddingBagConfig(num_embeddings=4, embedding_dim=D, name="t", data_type=dt)
                ]
            )

    def test_bit_order_int4(self):
        w = torch.arange(16, dtype=torch.float32).unsqueeze(0)
        packed = quantize_rowwise_nbit(w, 4)
        assert packed.shape == (1, 16)
        expect = bytes.fromhex("1032547698BADCFE" "003C0000" "00000000")
        assert bytes(packed[0].tolist()) == expect

    def test_bit_order_int2(self):
        w = torch.tensor([[0.0, 1.0, 2.0, 3.0] * 4])
        packed = quantize_rowwise_nbit(w, 2)
        assert packed.shape == (1, 16)
        expect = bytes.fromhex("E4E4E4E4" "003C0000" "0000000000000000")
        assert bytes(packed[0].tolist()) == expect

    @pytest.mark.parametrize(
        "bits,D", [(4, 8), (4, 16), (4, 64), (4, 128), (4, 264), (2, 16), (2, 64), (2, 128)]
    )
    def test_roundtrip_error_bound(self, bits, D):
        for name, w in roundtrip_inputs(200, D).items():
            packed = quantize_rowwise_nbit(w, bits)
            assert packed.shape == (200, nbit_row_stride(D, bits))
            cb = D * bits // 8
            assert not packed[:, cb + 4 :].any(), f"{name}: padding not zero"
            deq = dequantize_rowwise_nbit(packed, D, bits)
            err = (deq - w).abs().max(dim=1).values
            bound = row_bound(w, packed, bits)
            ratio = float((err / bound).max())
            print(f"bits={bits} D={D} {name}: worst err/bound {ratio:.4f}")
            assert (err <= bound).all(), f"{name}: worst err/bound {ratio}"

    @pytest.mark.parametrize("mode", ["sum", "mean", "weighted"])
    def test_mixed_ebc_close_to_float(self, mode):
        pooling = PoolingType.MEAN if mode == "mean" else PoolingType.SUM
        weighted = mode == "weighted"
        ebc = mixed_float_ebc(pooling, weighted)
        qebc = QuantEBC.from_float(ebc, per_table_weight_dtype=mixed_dtypes())
        assert [c.data_type for c in qebc.embedding_bag_configs()] == [s[2] for s in MIXED]
        kjt = make_kjt([f for s in MIXED for f in s[3]], MIXED_ROWS, MIXED_B, weighted)
        out_f = ebc(kjt).values().detach()
        out_q = qebc(kjt).values()
        assert out_q.shape == out_f.shape == (MIXED_B, 20 + 8 + 16 + 264 * 2 + 128)
        tol = ebc_tolerance(qebc, ebc, kjt, mode == "mean", weighted)
        err = (out_q - out_f).abs()
        assert (err <= tol).all(), f"worst excess {float((err - tol).max())}"
        assert float(err.max()) > 0  # the comparison is not vacuous

    def test_quant_ec_sequence(self):
        ec = seq_float_ec()
        qec = QuantEC.from_float(ec, per_table_weight_dtype=mixed_dtypes(SEQ))
        assert [c.data_type for c in qec.embedding_configs()] == [DataType.INT4, DataType.INT2]
        kjt = seq_kjt()
        out_f = ec(kjt)
        out_q = qec(kjt)
        assert out_q["fe"].values().shape == (0, 32)
        jts = kjt.to_dict()
        for t, (name, D, dt, feats) in enumerate(SEQ):
            w = ec.embeddings[name].weight.detach()
            bound = row_bound(w, qec._tbe.packed_table(t), BITS_OF[dt])
            for f in feats:
                idx = jts[f].values()
                err = (out_q[f].values() - out_f[f].values()).abs()
                assert err.shape == (idx.numel(), D)
                assert (err <= bound[idx].unsqueeze(1)).all()
                assert torch.equal(out_q[f].lengths(), out_f[f].lengths())

    def test_quantize_inference_model_per_table(self):
        model = small_dlrm()
        w0 = model.sparse_arch.embedding_bag_collection.embedding_bags["t0"].weight.detach().clone()
        quantize_inference_model(model, per_table_weight_dtype={"t0": DataType.INT4})
        q = model.sparse_arch.embedding_bag_collection
        assert isinstance(q, QuantEBC)
        assert [c.data_type for c in q.embedding_bag_configs()] == [DataType.INT4, DataType.INT8]
        assert q._tbe.qweights.numel() == 50 * nbit_row_stride(8, 4) + 50 * int8_row_stride(8)
        assert torch.equal(q._tbe.packed_table(0), quantize_rowwise_nbit(w0, 4))

    def test_quantize_inference_model_default_is_int8_bytes(self):
        model = small_dlrm()
        ebc = model.sparse_arch.embedding_bag_collection
        expect = torch.cat(
            [quantize_rowwise_int8(ebc.embedding_bags[n].weight.detach()).reshape(-1)
             for n in ("t0", "t1")]
        )
        quantize_inference_model(model)
        q = model.sparse_arch.embedding_bag_collection
        assert [c.data_type for c in q.embedding_bag_configs()] == [DataType.INT8, DataType.INT8]
        assert torch.equal(q._tbe.qweights, expect)

    def test_quantize_inference_model_weight_dtype(self):
        model = small_dlrm()
        quantize_inference_model(model, weight_dtype=DataType.INT4)
        q = model.sparse_arch.embedding_bag_collection
        assert [c.data_type for c in q.embedding_bag_configs()] == [DataType.INT4, DataType.INT4]
        assert q._tbe.qweights.numel() == 2 * 50 * nbit_row_stride(8, 4)
        # D=8 is not packable at 2 bits: the error surfaces at construction
        with pytest.raises(ValueError):
            quantize_inference_model(small_dlrm(), weight_dtype=DataType.INT2)

    def test_state_dict_roundtrip(self):
        ebc = mixed_float_ebc(specs=MIXED[1:4])
        q = QuantEBC.from_float(ebc, weight_dtype=DataType.INT4)
        fresh = QuantEBC(tables=q.embedding_bag_configs())
        assert not torch.equal(fresh._tbe.qweights, q._tbe.qweights)
        fresh.load_state_dict(q.state_dict())
        kjt = make_kjt([f for s in MIXED[1:4] for f in s[3]], MIXED_ROWS, MIXED_B)
        assert torch.equal(fresh(kjt).values(), q(kjt).values())


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


def gpu_copy_of(q_cpu, make):
    """A GPU module holding exactly q_cpu's packed bytes."""
    q_gpu = make()
    q_gpu._tbe.to(torch.device("cuda"))
    q_gpu._tbe.qweights.data.copy_(q_cpu._tbe.qweights.data.cuda())
    return q_gpu


@pytest.mark.gpu
class TestNbitGpu:
    @pytest.mark.parametrize("R", [1, 100])
    @pytest.mark.parametrize("bits,D", [(4, 8), (4, 64), (4, 264), (2, 16), (2, 64)])
    def test_quantize_kernel_matches_cpu(self, bits, D, R):
        g = torch.Generator().manual_seed(R * 1000 + D + bits)
        w = torch.randn(R, D, generator=g)
        if R > 1:
            w[R // 2] = 0.37  # one constant row
            w[1] = 100 * torch.rand(D, generator=g) - 20
        ref = quantize_rowwise_nbit(w, bits)
        got = quantize_rowwise_nbit(w.cuda(), bits)
        torch.cuda.synchronize()
        got = got.cpu()
        assert got.shape == ref.shape and got.dtype == torch.uint8
        cb = D * bits // 8
        # scale, bias and padding: bytewise
        assert torch.equal(got[:, cb:], ref[:, cb:])
        # a tie may round either way: codes within 1 everywhere
        diff = (
            unpack_codes_nbit(got, D, bits).int() - unpack_codes_nbit(ref, D, bits).int()
        ).abs()
        print(f"bits={bits} D={D} R={R}: codes differing {int((diff > 0).sum())}, max {int(diff.max())}")
        assert int(diff.max()) <= 1
        err = (dequantize_rowwise_nbit(got, D, bits) - w).abs().max(dim=1).values
        bound = row_bound(w, got, bits)
        assert (err <= bound).all(), f"worst err/bound {float((err / bound).max())}"

    @pytest.mark.parametrize("mode", ["sum", "mean", "weighted"])
    def test_mixed_pooled_matches_cpu(self, mode):
        pooling = PoolingType.MEAN if mode == "mean" else PoolingType.SUM
        weighted = mode == "weighted"
        ebc = mixed_float_ebc(pooling, weighted)
        make = lambda: QuantEBC.from_float(ebc, per_table_weight_dtype=mixed_dtypes())
        q_cpu = make()
        q_gpu = gpu_copy_of(q_cpu, make)
        kjt = make_kjt([f for s in MIXED for f in s[3]], MIXED_ROWS, MIXED_B, weighted)
        out_c = q_cpu(kjt).values()
        out_g = q_gpu(kjt.to(torch.device("cuda"))).values()
        torch.cuda.synchronize()
        torch.testing.assert_close(out_g.cpu(), out_c, atol=1e-4, rtol=1e-4)

    @pytest.mark.parametrize(
        "D,tables,rows,B",
        [(128, 2, 30, 3), (1032, 1, 5, 2)],  # 16 words; 129 words: multi-chunk, ragged tail
    )
    def test_uniform_int4_pooled_matches_cpu(self, D, tables, rows, B):
        specs = [(f"u{i}", D, DataType.INT4, [f"g{i}"]) for i in range(tables)]
        ebc = mixed_float_ebc(specs=specs, rows=rows)
        make = lambda: QuantEBC.from_float(ebc, weight_dtype=DataType.INT4)
        q_cpu = make()
        q_gpu = gpu_copy_of(q_cpu, make)
        kjt = make_kjt([f"g{i}" for i in range(tables)], rows, B)
        if tables == 1:  # keep some bag non-empty
            kjt = KeyedJaggedTensor(
                keys=["g0"], values=torch.tensor([4, 0, 2]), lengths=torch.tensor([2, 1]), stride=B
            )
        out_c = q_cpu(kjt).values()
        out_g = q_gpu(kjt.to(torch.device("cuda"))).values()
        torch.cuda.synchronize()
        assert float(out_c.abs().max()) > 0
        torch.testing.assert_close(out_g.cpu(), out_c, atol=1e-4, rtol=1e-4)

    def test_nbit_ops_at_8_bits_match_int8_ops(self):
        dev = torch.device("cuda")
        specs = [("a", 12, 20), ("b", 9, 128)]
        tbe = QuantTableBatchedEmbeddingBags(specs, device=dev)
        torch.manual_seed(0)
        for i, (_, rows, dim) in enumerate(specs):
            tbe.load_float_table(i, torch.randn(rows, dim))
        bits = torch.tensor([8, 8], dtype=torch.int32, device=dev)
        B = 4
        g = torch.Generator().manual_seed(2)
        lengths = torch.randint(0, 4, (2 * B,), generator=g)
        indices = torch.cat(
            [torch.randint(0, specs[i // B][1], (int(l),), generator=g)
             for i, l in enumerate(lengths)]
        ).to(dev)
        offsets = torch.zeros(2 * B + 1, dtype=torch.int64)
        torch.cumsum(lengths, 0, out=offsets[1:])
        offsets = offsets.to(dev)
        psw = torch.rand(indices.numel(), generator=g).to(dev)
        for w in (tbe._empty_f, psw):
            for mean in (False, True):
                a = torch.ops.trec_amd.tbe_forward_pooled_int8(
                    tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t,
                    tbe._d_out_offsets, indices, offsets, w, B, 148, 128, mean)
                b = torch.ops.trec_amd.tbe_forward_pooled_nbit(
                    tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t,
                    tbe._d_out_offsets, indices, offsets, w, B, 148, 32, mean)
                torch.cuda.synchronize()
                torch.testing.assert_close(b, a, atol=1e-6, rtol=1e-6)
        # sequence ops: output rows are 128 wide, a D=20 row fills its first 20 columns
        fvo = offsets[::B][:3].contiguous()
        a = torch.ops.trec_amd.tbe_forward_seq_int8(
            tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t, fvo,
            indices, 128, 128)
        b = torch.ops.trec_amd.tbe_forward_seq_nbit(
            tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t, fvo,
            indices, 128, 32)
        torch.cuda.synchronize()
        n0 = int(fvo[1])
        assert 0 < n0 < indices.numel()
        torch.testing.assert_close(b[:n0, :20], a[:n0, :20], atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(b[n0:], a[n0:], atol=1e-6, rtol=1e-6)

    def test_op_rejects_bad_dim(self):
        with pytest.raises(RuntimeError):
            torch.ops.trec_amd.quantize_rowwise_nbit(torch.zeros(2, 12, device="cuda"), 4)
        with pytest.raises(RuntimeError):
            torch.ops.trec_amd.quantize_rowwise_nbit(torch.zeros(2, 16, device="cuda"), 8)

    def test_seq_matches_cpu(self):
        ec = seq_float_ec()
        make = lambda: QuantEC.from_float(ec, per_table_weight_dtype=mixed_dtypes(SEQ))
        q_cpu = make()
        q_gpu = gpu_copy_of(q_cpu, make)
        kjt = seq_kjt()
        out_c = q_cpu(kjt)
        out_g = q_gpu(kjt.to(torch.device("cuda")))
        torch.cuda.synchronize()
        assert sum(v.values().numel() for v in out_c.values()) > 0
        for k in out_c:
            torch.testing.assert_close(
                out_g[k].values().cpu(), out_c[k].values(), atol=1e-4, rtol=1e-4
            )

    def test_uvm_matches_device(self):
        """QUANT_UVM at INT4: pinned-host packed tables match HBM tables."""
        specs = [("t0", 50, 64), ("t1", 30, 128)]
        dts = [DataType.INT4, DataType.INT4]
        dev = QuantTableBatchedEmbeddingBags(specs, device=torch.device("cuda"), weight_dtypes=dts)
        uvm = QuantTableBatchedEmbeddingBags(
            specs, device=torch.device("cuda"), location="managed", weight_dtypes=dts
        )
        assert not uvm.qweights.is_cuda and uvm.qweights.is_pinned()
        torch.manual_seed(0)
        for i, (n, rows, dim) in enumerate(specs):
            dev.load_float_table(i, torch.randn(rows, dim))
            uvm.packed_table(i).copy_(dev.packed_table(i).cpu())  # identical packed bytes
        B = 8
        g = torch.Generator().manual_seed(1)
        lengths = torch.randint(0, 4, (2 * B,), generator=g)
        indices = torch.cat(
            [torch.randint(0, specs[i // B][1], (int(l),), generator=g)
             for i, l in enumerate(lengths)]
        )
        offsets = torch.zeros(2 * B + 1, dtype=torch.int64)
        torch.cumsum(lengths, 0, out=offsets[1:])
        out_dev = dev(indices.cuda(), offsets.cuda())
        out_uvm = uvm(indices.cuda(), offsets.cuda())
        torch.cuda.synchronize()
        assert float(out_dev.abs().max()) > 0
        assert torch.equal(out_dev, out_uvm)

    def test_end_to_end_from_float_on_gpu(self):
        """GPU quantiser feeds the GPU lookup; compared with the float EBC."""
        # 8 and 4 lane units: the narrowest (8-lane) slot of the pooled kernel
        specs = [("e0", 64, DataType.INT4, ["h0"]), ("e1", 32, DataType.INT4, ["h1"])]
        ebc = mixed_float_ebc(specs=specs)
        kjt = make_kjt(["h0", "h1"], MIXED_ROWS, MIXED_B)
        out_f = ebc(kjt).values().detach()
        ebc.to(torch.device("cuda"))
        qebc = QuantEBC.from_float(ebc, weight_dtype=DataType.INT4)
        assert qebc._tbe.qweights.is_cuda
        out_q = qebc(kjt.to(torch.device("cuda"))).values()
        torch.cuda.synchronize()
        tol = ebc_tolerance(qebc, ebc, kjt, False, False)
        err = (out_q.cpu() - out_f).abs()
        assert (err <= tol).all(), f"worst excess {float((err - tol).max())}"
        assert float(err.max()) > 0
