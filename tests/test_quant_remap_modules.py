"""``bounds_check`` / ``index_remapping`` up the stack: quant EBC / EC
``from_float``, ``quantize_inference_model``, the ITEP helper, the config
field and the host-side errors.

The oracle is the quantized module built from the same float tables without
pruning: it quantises the same float rows with the same quantiser, so a kept
id reads the same bytes and the pooled sums are bit-identical once the dropped
ids are taken out of its input. Out-of-range ids follow the rule of
tests/test_quant_remap.py: none negative on the first table, none past the
end on the last."""

import pytest
import torch
import torch.nn as nn

from torchrec_amd.inference import quantize_inference_model
from torchrec_amd.modules.embedding_configs import (
    BaseEmbeddingConfig,
    DataType,
    EmbeddingBagConfig,
    EmbeddingConfig,
)
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection, EmbeddingCollection
from torchrec_amd.modules.itep_modules import GenericITEPModule, ITEPEmbeddingBagCollection
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEBC,
    EmbeddingCollection as QuantEC,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

gpu = pytest.mark.gpu
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=gpu)]

# logical rows, dim, format, remap (None: not pruned)
TABLES = {
    "u0": (9, 20, DataType.INT8, torch.tensor([3, -1, 0, -1, 4, -1, 1, -1, 2], dtype=torch.int32)),
    "u1": (7, 8, DataType.INT4, None),
    "u2": (6, 16, DataType.INT2, torch.tensor([-1, 1, -1, -1, 0, -1])),
}
REMAPS = {n: t[3] for n, t in TABLES.items() if t[3] is not None}
DTYPES = {n: t[2] for n, t in TABLES.items()}
# per table B=3 bags of logical ids: mixed, dropped only, empty
BAGS = {
    "u0": [[2, 1, 9, 8, 10], [3, 10, 9], []],
    "u1": [[0, -1, 6, 8], [7, -2], []],
    "u2": [[4, 0, -1, 1, -2], [5, -1], []],
}


def float_ebc(device):
    torch.manual_seed(3)
    tables = [
        EmbeddingBagConfig(num_embeddings=r, embedding_dim=d, name=n, feature_names=[f"f_{n}"])
        for n, (r, d, _, _) in TABLES.items()
    ]
    return EmbeddingBagCollection(tables=tables, device=torch.device(device))


def make_kjt(bags, device):
    keys = [f"f_{n}" for n in bags]
    values = torch.tensor([i for n in bags for bag in bags[n] for i in bag], dtype=torch.int64)
    lengths = torch.tensor([len(bag) for n in bags for bag in bags[n]])
    return KeyedJaggedTensor(keys=keys, values=values, lengths=lengths, stride=3).to(
        torch.device(device)
    )


def surviving_bags():
    """BAGS without the dropped ids (the ids stay logical: the oracle is not pruned)."""
    out = {}
    for n, (rows, _, _, remap) in TABLES.items():
        keep = lambda i: 0 <= i < rows and (remap is None or int(remap[i]) >= 0)
        out[n] = [[i for i in bag if keep(i)] for bag in BAGS[n]]
    return out


def out_of_range_counts():
    return [sum(not 0 <= i < TABLES[n][0] for bag in BAGS[n] for i in bag) for n in TABLES]


@pytest.mark.parametrize("device", DEVICES)
def test_ebc_from_logical_float_table(device):
    ebc = float_ebc(device)
    full = QuantEBC.from_float(ebc, per_table_weight_dtype=DTYPES)
    q = QuantEBC.from_float(ebc, per_table_weight_dtype=DTYPES, index_remapping=REMAPS)
    assert [s[1] for s in q._tbe._specs] == [5, 7, 2]
    cfg = {t.name: t for t in q.embedding_bag_configs()}
    assert cfg["u0"].num_embeddings == 9 and cfg["u0"].num_embeddings_post_pruning == 5
    assert cfg["u1"].num_embeddings == 7 and cfg["u1"].num_embeddings_post_pruning is None
    got = q(make_kjt(BAGS, device)).values()
    want = full(make_kjt(surviving_bags(), device)).values()
    assert torch.equal(got, want) and float(want.abs().max()) > 0
    assert int(got[1:].count_nonzero()) == 0  # bags of dropped ids only, and empty bags
    assert q._tbe.out_of_range_counts().tolist() == out_of_range_counts()


@pytest.mark.parametrize("device", DEVICES)
def test_quantize_inference_model(device):
    """An EBC and an EC in one model; index_remapping names tables of both."""

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.ebc = float_ebc(device)
            torch.manual_seed(5)
            self.ec = EmbeddingCollection(
                tables=[
                    EmbeddingConfig(num_embeddings=6, embedding_dim=16, name="s0", feature_names=["g0"]),
                    EmbeddingConfig(num_embeddings=5, embedding_dim=16, name="s1", feature_names=["g1"]),
                ],
                device=torch.device(device),
            )

    remaps = dict(REMAPS, s0=torch.tensor([-1, 1, -1, 2, 0, -1]))
    # the quant EC is built on the CPU; serving moves the model (shard_quant_model)
    full = quantize_inference_model(Model(), per_table_weight_dtype=DTYPES).to(device)
    q = quantize_inference_model(
        Model(), per_table_weight_dtype=DTYPES, bounds_check=True, index_remapping=remaps
    ).to(device)
    assert isinstance(q.ebc, QuantEBC) and isinstance(q.ec, QuantEC)
    assert q.ebc._tbe._checked and q.ec._tbe._checked and not full.ebc._tbe._checked
    got = q.ebc(make_kjt(BAGS, device)).values()
    assert torch.equal(got, full.ebc(make_kjt(surviving_bags(), device)).values())
    # sequence: s0 is pruned (6 -> 3), s1 only bounds-checked
    seq = {"g0": [[4, 0, 6], [1, 7, 3], []], "g1": [[4, -1, 0], [-2, 2], []]}
    kjt = KeyedJaggedTensor(
        keys=["g0", "g1"],
        values=torch.tensor([i for k in seq for bag in seq[k] for i in bag]),
        lengths=torch.tensor([len(bag) for k in seq for bag in seq[k]]),
        stride=3,
    ).to(torch.device(device))
    out = q.ec(kjt)
    kept = {"g0": [4, 1, 3], "g1": [4, 0, 2]}
    ref = full.ec(
        KeyedJaggedTensor(
            keys=["g0", "g1"], values=torch.tensor(kept["g0"] + kept["g1"]),
            lengths=torch.tensor([3, 0, 0, 3, 0, 0]), stride=3,
        ).to(torch.device(device))
    )
    for k, dropped in (("g0", [1, 2, 4]), ("g1", [1, 3])):
        rows = out[k].values()
        mask = torch.zeros(rows.shape[0], dtype=torch.bool)
        mask[dropped] = True
        assert int(rows[mask].count_nonzero()) == 0
        assert torch.equal(rows[~mask], ref[k].values()) and float(rows.abs().max()) > 0
    assert q.ec._tbe.out_of_range_counts().tolist() == [2, 2]
    # a custom mapping with the original from_float signature still works unset
    class OldStyle(QuantEBC):
        @classmethod
        def from_float(cls, module, output_dtype=torch.float32):
            return super().from_float(module, output_dtype=output_dtype)

    old = quantize_inference_model(Model(), {EmbeddingBagCollection: OldStyle})
    assert isinstance(old.ebc, OldStyle) and isinstance(old.ec, EmbeddingCollection)


@pytest.mark.parametrize("device", DEVICES)
def test_itep_physical_float_table(device):
    """A float EBC trained under ITEP holds PHYSICAL rows; with the module's
    own eval-time mapping the quant EBC serves what the ITEP wrapper computes
    in eval over the same quantized rows. Many ids share the last row."""
    unpruned, pruned = {"p0": 12, "p1": 9}, {"p0": 4, "p1": 3}
    torch.manual_seed(11)
    ebc = EmbeddingBagCollection(
        tables=[
            EmbeddingBagConfig(num_embeddings=pruned[n], embedding_dim=8, name=n, feature_names=[f"f_{n}"])
            for n in unpruned
        ],
        device=torch.device(device),
    )
    itep = GenericITEPModule(unpruned, pruned_hash_sizes=pruned).to(torch.device(device))
    # a lookup that is not the initial one: ids 7 and 10 own rows 0 and 2 of p0
    itep._lookup_p0[0], itep._lookup_p0[2] = -1, -1
    itep._lookup_p0[7], itep._lookup_p0[10] = 0, 2
    remaps = {n: itep.index_remapping(n) for n in unpruned}
    assert int(remaps["p0"].min()) == 0 and remaps["p0"].tolist().count(3) == 9
    q = QuantEBC.from_float(ebc, index_remapping=remaps)
    assert [s[1] for s in q._tbe._specs] == [4, 3]
    assert [t.num_embeddings for t in q.embedding_bag_configs()] == [12, 9]
    wrapper = ITEPEmbeddingBagCollection(QuantEBC.from_float(ebc), itep).eval()
    bags = {"p0": [[7, 0, 11, 3], [10], []], "p1": [[8, 0], [], [2, 2, 5]]}
    kjt = make_kjt(bags, device)
    got, want = q(kjt).values(), wrapper(kjt).values()
    assert torch.equal(got, want) and float(want.abs().max()) > 0
    # ids past the unpruned space are dropped, not clamped (p0 is not the last table)
    extra = make_kjt({"p0": [[12, 13], [], []], "p1": [[-1], [], []]}, device)
    assert int(q(extra).values().count_nonzero()) == 0
    assert q._tbe.out_of_range_counts().tolist() == [2, 1]


def test_host_side_errors():
    ebc = float_ebc("cpu")
    mk = lambda **remaps: QuantEBC.from_float(ebc, per_table_weight_dtype=DTYPES, index_remapping=remaps)
    # non-injective remap on a logical table: ids 0 and 2 both on row 0
    with pytest.raises(ValueError, match="table u2.*row 0"):
        mk(u2=torch.tensor([0, 1, 0, -1, -1, -1]))
    # a physical row nobody maps to
    with pytest.raises(ValueError, match="table u2.*row 1"):
        mk(u2=torch.tensor([0, -1, 2, -1, -1, -1]))
    # neither the logical nor the physical row count
    with pytest.raises(ValueError, match="table u2.*6 rows"):
        mk(u2=torch.tensor([0, 1, -1, -1]))
    with pytest.raises(ValueError, match="table u2.*-3"):
        mk(u2=torch.tensor([0, 1, -3, -1, -1, -1]))
    with pytest.raises(ValueError, match="table u2.*int32 or int64"):
        mk(u2=torch.tensor([0.0, 1.0, -1.0, -1.0, -1.0, -1.0]))

    def cfg(**kw):
        return EmbeddingBagConfig(embedding_dim=8, name="v", feature_names=["f"], **kw)

    remap = torch.tensor([1, -1, 0, -1])
    ok = QuantEBC([cfg(num_embeddings=4, num_embeddings_post_pruning=2)], index_remapping={"v": remap})
    assert ok._tbe._specs[0][1] == 2 and ok._tbe._logical_rows == [4]
    with pytest.raises(ValueError, match="table v.*post_pruning=3"):
        QuantEBC([cfg(num_embeddings=4, num_embeddings_post_pruning=3)], index_remapping={"v": remap})
    with pytest.raises(ValueError, match="table v.*post_pruning=2"):
        QuantEBC([cfg(num_embeddings=4, num_embeddings_post_pruning=2)])
    with pytest.raises(ValueError, match=r"table v.*\[5\]"):  # wrong length
        QuantEBC([cfg(num_embeddings=5)], index_remapping={"v": remap})
    with pytest.raises(KeyError, match="nope"):
        QuantEBC([cfg(num_embeddings=4)], index_remapping={"nope": remap})
    with pytest.raises(ValueError, match="table v.*post_pruning=3"):
        QuantEC(
            [EmbeddingConfig(num_embeddings=4, embedding_dim=8, name="v", feature_names=["f"],
                             num_embeddings_post_pruning=3)],
            index_remapping={"v": remap},
        )


def test_config_field():
    for cls in (BaseEmbeddingConfig, EmbeddingBagConfig, EmbeddingConfig):
        c = cls(num_embeddings=10, embedding_dim=4, name="t")
        assert c.num_embeddings_post_pruning is None
        c = cls(num_embeddings=10, embedding_dim=4, name="t", num_embeddings_post_pruning=6)
        assert c.num_embeddings_post_pruning == 6 and c.num_embeddings == 10
