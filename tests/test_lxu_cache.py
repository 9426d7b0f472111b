"""lxu cache (``cache.hip``, ``EmbeddingLocation.MANAGED_CACHING``).

A. ``LxuCacheModel``: the cache policy in plain numpy, with CPU self-tests.
B. The populate / lookup / flush kernels against that model, bitwise.
C. Every forward / backward path of a cached module against a device-resident
   module, under inline population and under prefetch-ahead.

The pipeline test that goes with these lives in ``test_gpu_e2e.py`` and takes
its batches and their eviction pre-condition from here.
"""

import numpy as np
import pytest
import torch

from torchrec_amd.ops.tbe import EmbeddingLocation, PoolingMode, TableBatchedEmbeddingBags

WAYS = 32


# ---------------------------------------------------------------------------
# A. the model
# ---------------------------------------------------------------------------


class LxuCacheModel:
    """The policy of ``lxu_cache_populate_kernel`` and friends, one id at a time.

    ``host_table_rows`` is one ``[rows_t, D_t]`` array per table; the model
    keeps its own copy. Linear ids index the concatenation of the tables.
    """

    def __init__(self, sets, max_D, host_table_rows):
        self.sets = int(sets)
        self.max_D = int(max_D)
        self.host = [np.array(t, dtype=np.float32, copy=True) for t in host_table_rows]
        self.row_offsets = np.cumsum([0] + [t.shape[0] for t in self.host]).astype(np.int64)
        n = self.sets * WAYS
        self.tags = np.full(n, -1, dtype=np.int64)
        self.lru = np.zeros(n, dtype=np.int64)
        self.cache_rows = np.zeros((n, self.max_D), dtype=np.float32)
        self.timestamp = 0

    # -- addressing ---------------------------------------------------------

    def locate(self, lin):
        lin = int(lin)
        assert 0 <= lin < self.row_offsets[-1], lin
        t = int(np.searchsorted(self.row_offsets, lin, side="right")) - 1
        return t, lin - int(self.row_offsets[t])

    def dim(self, lin):
        return self.host[self.locate(lin)[0]].shape[1]

    def host_flat(self):
        return np.concatenate([t.reshape(-1) for t in self.host])

    # -- the three operations -----------------------------------------------

    def populate(self, ids):
        """One batch: unique ids ascending, each set visited by one owner.
        Returns the ids evicted by this call, in eviction order."""
        uniq = np.unique(np.asarray(ids, dtype=np.int64))
        evicted = []
        if uniq.size == 0:
            return evicted
        self.timestamp += 1
        for lin in uniq:
            base = int(lin % self.sets) * WAYS
            tags = self.tags[base : base + WAYS]
            hit = np.nonzero(tags == lin)[0]
            if hit.size:
                self.lru[base + hit[0]] = self.timestamp
                continue
            empty = np.nonzero(tags == -1)[0]
            if empty.size:
                way = int(empty[0])
            else:
                way = int(np.argmin(self.lru[base : base + WAYS]))  # lowest way on ties
            slot = base + way
            old = int(self.tags[slot])
            if old >= 0:
                t, r = self.locate(old)
                self.host[t][r, :] = self.cache_rows[slot, : self.host[t].shape[1]]
                evicted.append(old)
            t, r = self.locate(lin)
            self.cache_rows[slot, : self.host[t].shape[1]] = self.host[t][r]
            self.tags[slot] = lin
            self.lru[slot] = self.timestamp
        return evicted

    def lookup(self, ids):
        out = np.full(len(ids), -1, dtype=np.int32)
        for i, lin in enumerate(np.asarray(ids, dtype=np.int64)):
            base = int(lin % self.sets) * WAYS
            hit = np.nonzero(self.tags[base : base + WAYS] == lin)[0]
            if hit.size:
                out[i] = base + hit[0]
        return out

    def flush(self):
        for slot in np.nonzero(self.tags >= 0)[0]:
            t, r = self.locate(self.tags[slot])
            self.host[t][r, :] = self.cache_rows[slot, : self.host[t].shape[1]]

    # -- what training does to a row ------------------------------------------

    def write(self, lin, values):
        """A row's current copy: its slot while cached, else the host row."""
        slot = int(self.lookup([lin])[0])
        if slot >= 0:
            self.cache_rows[slot, : len(values)] = values
        else:
            t, r = self.locate(lin)
            self.host[t][r, :] = values


def _tables(rows_dims, seed):
    g = np.random.default_rng(seed)
    return [g.standard_normal((r, d)).astype(np.float32) for r, d in rows_dims]


def _check_invariants(m):
    valid = m.tags[m.tags >= 0]
    assert len(np.unique(valid)) == len(valid), "a tag appears twice"
    slots = np.nonzero(m.tags >= 0)[0]
    assert np.array_equal(m.lookup(m.tags[slots]), slots.astype(np.int32))
    assert np.array_equal(slots // WAYS, m.tags[slots] % m.sets), "tag in a foreign set"
    absent = np.setdiff1d(np.arange(m.row_offsets[-1]), valid)
    assert (m.lookup(absent) == -1).all()


class TestModel:
    @pytest.mark.parametrize("sets", [1, 3])
    def test_invariants_and_flush_against_last_written_value(self, sets):
        rows_dims = [(70, 8), (50, 4)]
        tables = _tables(rows_dims, 0)
        m = LxuCacheModel(sets, 8, tables)
        truth = {}  # id -> last written value
        g = np.random.default_rng(1)
        n_evicted = 0
        for step in range(40):
            ids = g.integers(0, 120, size=g.integers(1, 60))
            n_evicted += len(m.populate(ids))
            _check_invariants(m)
            for lin in g.choice(ids, size=min(5, len(ids)), replace=False):
                v = g.standard_normal(m.dim(lin)).astype(np.float32)
                m.write(lin, v)
                truth[int(lin)] = v
        assert (m.tags >= 0).all() and n_evicted > 100 and len(truth) > 50
        m.flush()
        want = [t.copy() for t in tables]
        for lin, v in truth.items():
            t, r = m.locate(lin)
            want[t][r] = v
        for got, w in zip(m.host, want):
            assert np.array_equal(got, w)

    def test_victims_empty_ways_then_oldest_lowest_way(self):
        m = LxuCacheModel(1, 4, _tables([(200, 4)], 0))
        assert m.populate(np.arange(40)) == [0] + list(range(32, 39))
        # ids 32..39 all land in way 0: every stamp ties, the lowest way loses
        assert m.tags[0] == 39 and np.array_equal(m.tags[1:], np.arange(1, 32))
        assert (m.lookup(np.arange(32, 39)) == -1).all() and m.lookup([0])[0] == -1
        m.populate(np.arange(1, 11))  # hits only: stamps of ways 1..10 move
        assert np.array_equal(m.lru, np.where((np.arange(32) >= 1) & (np.arange(32) <= 10), 2, 1))
        ev = m.populate(np.arange(100, 120))
        # oldest stamp 1: way 0, then ways 11..29
        assert ev == [39] + list(range(11, 30))

    def test_empty_batch_is_a_no_op(self):
        m = LxuCacheModel(1, 4, _tables([(10, 4)], 0))
        assert m.populate([]) == [] and m.timestamp == 0 and (m.tags == -1).all()
        assert m.lookup([]).shape == (0,) and m.lookup([]).dtype == np.int32


# ---------------------------------------------------------------------------
# shared inputs of B
# ---------------------------------------------------------------------------

ONE_SET_SPECS = [("t0", 96, 64)]
THREE_SET_SPECS = [("t0", 300, 128), ("t1", 200, 64)]  # 500 rows * 0.2 = 100 -> 3 sets
THREE_SET_EDGE_IDS = [299, 300, 499, 0, 3, 297, 303, 498]


def single_feature_batch(ids):
    """One table, one bag per id."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    return ids, torch.arange(ids.numel() + 1, dtype=torch.int64)


def one_set_batches():
    return [
        np.arange(40) * 2,  # 40 unique ids in a 32-slot set
        np.concatenate([np.arange(1, 17) * 2, np.arange(1, 9) * 2]),  # pure hits (with dups)
        np.arange(20) * 2 + 1,  # 20 new ids
    ]


def three_set_batches():
    """Six batches, B=8, L=4 per feature -> (indices, offsets, linear ids)."""
    g = np.random.default_rng(5)
    B, L = 8, 4
    out = []
    for k in range(6):
        i0 = g.integers(0, 300, size=B * L)
        i1 = g.integers(0, 200, size=B * L)
        # table edges (the upper_bound_segment boundaries) and multiples of 3
        i0[:4] = [299, 0, 3, 297]
        i1[:4] = [0, 199, 3, 198]  # linear 300, 499, 303, 498
        if k % 2:
            i0[4:12] = i0[:8]  # duplicates: the unique list ends in a -1 run
        indices = np.concatenate([i0, i1])
        offsets = np.arange(0, 2 * B * L + 1, L)
        out.append((indices, offsets, np.concatenate([i0, i1 + 300])))
    return out


class TestPreconditionsB:
    def test_one_set_case(self):
        m = LxuCacheModel(1, 64, _tables([(96, 64)], 0))
        b0, b1, b2 = one_set_batches()
        host0 = m.host_flat().copy()
        ev = m.populate(b0)
        assert len(np.unique(b0)) == 40 and len(ev) == 8
        assert set(ev) <= set(b0.tolist())  # evicts rows of the same call
        assert (m.lookup(ev) == -1).all()
        assert np.array_equal(m.host_flat(), host0)  # clean rows: host unchanged
        tags = m.tags.copy()
        assert m.populate(b1) == [] and np.array_equal(m.tags, tags)
        assert len(m.populate(b2)) == 20

    def test_three_set_case(self):
        specs = THREE_SET_SPECS
        total = sum(s[1] for s in specs)
        assert max(1, max(WAYS, int(total * 0.2)) // WAYS) == 3
        m = LxuCacheModel(3, 128, _tables([(300, 128), (200, 64)], 0))
        n_ev = 0
        for _, _, lin in three_set_batches():
            assert set(THREE_SET_EDGE_IDS) <= set(lin.tolist())
            n_ev += len(m.populate(lin))
        assert n_ev > 0
        assert any(len(np.unique(lin)) < len(lin) for _, _, lin in three_set_batches())


# ---------------------------------------------------------------------------
# B. kernels against the model
# ---------------------------------------------------------------------------


def make_cached(specs, seed=0, **kw):
    tbe = TableBatchedEmbeddingBags(
        specs, optimizer="rowwise_adagrad", learning_rate=0.05, device=torch.device("cuda"),
        location=EmbeddingLocation.MANAGED_CACHING, cache_load_factor=0.2, **kw,
    )
    tables = _tables([(s[1], s[2]) for s in specs], seed)
    tbe.weights.copy_(torch.from_numpy(np.concatenate([t.reshape(-1) for t in tables])))
    return tbe, tables


def assert_state_equals_model(tbe, m, what):
    torch.cuda.synchronize()
    assert torch.equal(tbe.cache_tags.cpu(), torch.from_numpy(m.tags)), f"{what}: tags"
    assert torch.equal(tbe.cache_lru.cpu(), torch.from_numpy(m.lru)), f"{what}: lru"
    cw = tbe.cache_weights.cpu()
    for slot in np.nonzero(m.tags >= 0)[0]:
        D = m.dim(m.tags[slot])
        assert torch.equal(cw[slot, :D], torch.from_numpy(m.cache_rows[slot, :D])), (
            f"{what}: cache row of slot {slot} (id {m.tags[slot]})"
        )
    assert torch.equal(tbe.weights, torch.from_numpy(m.host_flat())), f"{what}: host table"


def train_some_rows(tbe, m, seed, count=6):
    """Overwrite some cached rows with fresh values, in the kernel's buffers and in
    the model: the write-back on eviction and flush then shows in the host table."""
    g = np.random.default_rng(seed)
    slots = np.nonzero(m.tags >= 0)[0]
    for slot in g.choice(slots, size=min(count, len(slots)), replace=False):
        D = m.dim(m.tags[slot])
        v = g.standard_normal(D).astype(np.float32)
        m.cache_rows[slot, :D] = v
        tbe.cache_weights[int(slot), :D] = torch.from_numpy(v).cuda()


@pytest.mark.gpu
class TestKernelsAgainstModel:
    def test_one_set_overflow_hits_then_lru_victims(self):
        tbe, tables = make_cached(ONE_SET_SPECS)
        assert tbe._cache_sets == 1 and tbe.cache_tags.numel() == WAYS
        m = LxuCacheModel(1, tbe.cache_weights.shape[1], tables)
        b0, b1, b2 = one_set_batches()
        host0 = tbe.weights.clone()

        loc = tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(b0)])
        ev = m.populate(b0)
        assert_state_equals_model(tbe, m, "overflow batch")
        assert torch.equal(loc.cpu(), torch.from_numpy(m.lookup(b0)))
        displaced = np.isin(b0, ev)
        assert displaced.sum() == 8 and (loc.cpu()[torch.from_numpy(displaced)] == -1).all()
        assert torch.equal(tbe.weights, host0)  # the displaced rows were clean

        train_some_rows(tbe, m, seed=1)
        loc = tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(b1)])
        tags_before = m.tags.copy()
        m.populate(b1)
        assert np.array_equal(m.tags, tags_before)
        assert_state_equals_model(tbe, m, "pure hits")
        assert torch.equal(loc.cpu(), torch.from_numpy(m.lookup(b1))) and (loc >= 0).all()

        train_some_rows(tbe, m, seed=2, count=12)
        loc = tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(b2)])
        m.populate(b2)
        assert_state_equals_model(tbe, m, "20 new ids")
        assert torch.equal(loc.cpu(), torch.from_numpy(m.lookup(b2)))
        assert not torch.equal(tbe.weights, host0)  # dirty victims were written back

    def test_three_sets_two_tables_edges_and_padding(self):
        tbe, tables = make_cached(THREE_SET_SPECS)
        assert tbe._cache_sets == 3 and tbe.cache_weights.shape[1] == 128
        m = LxuCacheModel(3, 128, tables)
        for k, (indices, offsets, lin) in enumerate(three_set_batches()):
            loc = tbe._populate_and_lookup(
                torch.from_numpy(indices).cuda(), torch.from_numpy(offsets).cuda()
            )
            m.populate(lin)
            assert_state_equals_model(tbe, m, f"batch {k}")
            assert torch.equal(loc.cpu(), torch.from_numpy(m.lookup(lin))), f"batch {k}: loc"
            train_some_rows(tbe, m, seed=10 + k)
        tbe.flush_cache()
        m.flush()
        assert_state_equals_model(tbe, m, "flush")

    def test_padding_never_inserts_the_sentinel(self):
        tbe, tables = make_cached(ONE_SET_SPECS)
        m = LxuCacheModel(1, 64, tables)
        ids = np.array([5, 5, 5, 9, 9, 0, 0, 95, 95, 95, 5, 0])  # 4 unique of 12
        loc = tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(ids)])
        m.populate(ids)
        assert_state_equals_model(tbe, m, "duplicates")
        tags, lru = tbe.cache_tags.cpu(), tbe.cache_lru.cpu()
        assert sorted(tags[tags != -1].tolist()) == [0, 5, 9, 95]
        assert (tags[4:] == -1).all() and (lru[4:] == 0).all()  # empty ways untouched
        assert torch.equal(loc.cpu(), torch.from_numpy(m.lookup(ids)))

    def test_empty_batch_is_a_no_op(self):
        tbe, tables = make_cached(ONE_SET_SPECS)
        m = LxuCacheModel(1, 64, tables)
        ids = np.arange(10)
        tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(ids)])
        m.populate(ids)
        loc = tbe._populate_and_lookup(
            torch.empty(0, dtype=torch.int64, device="cuda"),
            torch.zeros(9, dtype=torch.int64, device="cuda"),
        )
        assert loc.dtype == torch.int32 and loc.shape == (0,) and loc.is_cuda
        assert_state_equals_model(tbe, m, "empty batch")

    def test_flush_writes_back_and_leaves_the_cache_alone(self):
        tbe, tables = make_cached(ONE_SET_SPECS)
        m = LxuCacheModel(1, 64, tables)
        ids = np.arange(30) * 3
        tbe._populate_and_lookup(*[t.cuda() for t in single_feature_batch(ids)])
        m.populate(ids)
        train_some_rows(tbe, m, seed=3, count=10)
        before = [t.clone() for t in (tbe.cache_tags, tbe.cache_lru, tbe.cache_weights)]
        host_before = tbe.weights.clone()
        tbe.flush_cache()
        m.flush()
        assert_state_equals_model(tbe, m, "flush")
        assert not torch.equal(tbe.weights, host_before)
        for b, t in zip(before, (tbe.cache_tags, tbe.cache_lru, tbe.cache_weights)):
            assert torch.equal(b, t)


# ---------------------------------------------------------------------------
# C. every module path against a device-resident module
# ---------------------------------------------------------------------------

PAIR_SPECS = [("t0", 96, 64), ("t1", 64, 128)]  # 160 rows * 0.2 = 32 slots: one set
PAIR_B, PAIR_L = 8, 3
# per-batch id pools: 18 + 12 = 30 unique ids, consecutive batches share 3 + 2
POOL = ((96, 18, 15), (64, 12, 10))  # (rows, pool size, stride from batch to batch)


def pair_batch(k, bpf=(PAIR_B, PAIR_B)):
    """Batch k -> (indices, offsets, linear ids), every bag PAIR_L long."""
    g = np.random.default_rng(100 + k)
    parts, lin = [], []
    row0 = 0
    for (rows, size, stride), bags in zip(POOL, bpf):
        pool = (k * stride + np.arange(size)) % rows
        n = bags * PAIR_L
        idx = pool[g.permutation(max(n, size))[:n] % size]
        parts.append(idx)
        lin.append(idx + row0)
        row0 += rows
    indices = np.concatenate(parts).astype(np.int64)
    offsets = np.arange(0, indices.size + 1, PAIR_L, dtype=np.int64)
    return indices, offsets, np.concatenate(lin).astype(np.int64)


def pipeline_order(n, path="sum"):
    ev = [("prefetch", 0, path)]
    for i in range(n):
        if i + 1 < n:
            ev.append(("prefetch", i + 1, path))
        ev += [("fwd", i, path), ("bwd", i)]
    return ev


def inline_order(n, path="sum"):
    return [e for i in range(n) for e in (("fwd", i, path), ("bwd", i))]


PATHS = ["wsum", "wsum_grad", "mean", "vbe", "seq"]
VBE_BPF = (8, 5)

MIXED = {
    other: inline_order(2)
    + [("fwd", 2, other), ("bwd", 2), ("fwd", 3, other), ("bwd", 3), ("flush",)]
    + [("fwd", 4, "sum"), ("bwd", 4), ("fwd", 5, "sum"), ("bwd", 5)]
    for other in ("vbe8", "seq")
}
MIXED_PIPELINED = {
    other: [("prefetch", 0, "sum"), ("prefetch", 1, "sum"), ("fwd", 0, "sum"), ("bwd", 0),
            ("prefetch", 2, other), ("fwd", 1, "sum"), ("bwd", 1),
            ("prefetch", 3, other), ("fwd", 2, other), ("bwd", 2),
            ("prefetch", 4, "sum"), ("fwd", 3, other), ("bwd", 3), ("flush",),
            ("prefetch", 5, "sum"), ("fwd", 4, "sum"), ("bwd", 4), ("fwd", 5, "sum"), ("bwd", 5)]
    for other in ("vbe8", "seq")
}

SCHEDULES = {
    "pipeline_order": pipeline_order(5),
    "prefetch_between_fwd_and_bwd": [
        ("fwd", 0, "sum"), ("prefetch", 1, "sum"), ("bwd", 0), ("fwd", 1, "sum"), ("bwd", 1),
    ],
    "prefetch_two_ahead": [("prefetch", k, "sum") for k in range(3)] + inline_order(3),
    "unconsumed_prefetch": [
        ("prefetch", 0, "vbe8"), ("fwd", 0, "vbe8"), ("bwd", 0), ("fwd", 1, "sum"), ("bwd", 1),
    ],
}


def _bpf(path):
    return VBE_BPF if path == "vbe" else (PAIR_B, PAIR_B)


class TestPreconditionsC:
    """The schedules of C do displace rows that a pending batch uses."""

    def _model(self):
        return LxuCacheModel(1, 128, _tables([(96, 64), (64, 128)], 0))

    def test_batches_have_one_length_and_stay_in_range(self):
        for bpf in ((8, 8), VBE_BPF):
            for k in range(6):
                idx, off, lin = pair_batch(k, bpf)
                assert idx.size == sum(bpf) * PAIR_L == lin.size and off[-1] == idx.size
                n0 = bpf[0] * PAIR_L
                assert (idx[:n0] < 96).all() and (idx[n0:] < 64).all() and (idx >= 0).all()
                assert lin.max() < 160 and idx.size <= 100
        shared = len(set(pair_batch(0)[2]) & set(pair_batch(1)[2]))
        assert shared <= 6  # mostly disjoint

    def test_pipeline_order_displaces_the_current_batch(self):
        m = self._model()
        m.populate(pair_batch(0)[2])
        for i in range(4):
            ev = m.populate(pair_batch(i + 1)[2])  # prefetch(i+1) before fwd(i)
            assert len(set(ev) & set(pair_batch(i)[2].tolist())) >= 8, i
            assert (m.lookup(pair_batch(i)[2]) == -1).sum() >= 8

    def test_prefetch_between_fwd_and_bwd_displaces_the_forward_rows(self):
        m = self._model()
        m.populate(pair_batch(0)[2])
        ev = m.populate(pair_batch(1)[2])
        assert len(set(ev) & set(pair_batch(0)[2].tolist())) >= 8

    def test_prefetch_two_ahead_displaces_batch_zero(self):
        m = self._model()
        for k in range(3):
            m.populate(pair_batch(k)[2])
        assert len(set(pair_batch(0)[2][m.lookup(pair_batch(0)[2]) == -1].tolist())) >= 8

    def test_a_pooled_step_leaves_rows_a_later_path_uses(self):
        # mixed paths: rows of the pooled steps are still cached (and dirty)
        # when the VBE / sequence steps start, and these use some of them
        m = self._model()
        m.populate(pair_batch(0)[2])
        m.populate(pair_batch(1)[2])
        assert (m.lookup(pair_batch(2)[2]) >= 0).any()


def run_pair(schedule, pooling=PoolingMode.SUM):
    """Play ``schedule`` on a cached and on a device-resident module from the same
    standard-normal tables; compare every forward, the psw gradients and the end state."""
    dev = torch.device("cuda")
    common = dict(optimizer="rowwise_adagrad", learning_rate=0.05, device=dev, pooling_mode=pooling)
    ref = TableBatchedEmbeddingBags(PAIR_SPECS, **common)
    cached = TableBatchedEmbeddingBags(
        PAIR_SPECS, location=EmbeddingLocation.MANAGED_CACHING, cache_load_factor=0.2, **common
    )
    assert cached._uvm_caching and cached._cache_sets == 1 and cached.cache_tags.numel() == WAYS
    w0 = torch.from_numpy(
        np.concatenate([t.reshape(-1) for t in _tables([(96, 64), (64, 128)], 0)])
    )
    ref.weights.copy_(w0)
    cached.weights.copy_(w0)

    def inputs(k, path):
        idx, off, _ = pair_batch(k, _bpf(path))
        return torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev)

    def psw_for(k, n):
        g = torch.Generator().manual_seed(500 + k)
        return (torch.rand(n, generator=g) + 0.5).to(dev)

    def forward(mod, k, path):
        idx, off = inputs(k, path)
        psw = None
        if path in ("wsum", "wsum_grad"):
            psw = psw_for(k, idx.numel())
            if path == "wsum_grad":
                psw.requires_grad_()
        if path in ("vbe", "vbe8"):
            out = mod.forward_vbe(idx, off, list(_bpf(path)))
        elif path == "seq":
            out = mod._forward_seq(idx, off)
        else:
            out = mod(idx, off, psw)
        return out, psw

    # a sequence row of the narrower table fills its first 64 columns only
    n0 = PAIR_B * PAIR_L
    seq_valid = torch.ones(2 * n0, 128, dtype=torch.bool, device=dev)
    seq_valid[:n0, 64:] = False

    pending = {}
    for event in schedule:
        what = event[0]
        if what == "prefetch":
            _, k, path = event
            idx, off = inputs(k, path)
            if path == "vbe":  # variable batch: prefetch needs the bag layout
                cached.prefetch(idx, off, list(VBE_BPF))
            else:
                cached.prefetch(idx, off)
        elif what == "flush":
            cached.flush_cache()
        elif what == "fwd":
            _, k, path = event
            out_r, psw_r = forward(ref, k, path)
            out_c, psw_c = forward(cached, k, path)
            a, b = out_c.detach(), out_r.detach()
            if path == "seq":
                a, b = torch.where(seq_valid, a, 0.0), torch.where(seq_valid, b, 0.0)
            torch.testing.assert_close(a, b, atol=1e-5, rtol=1e-5, msg=lambda s: f"fwd({k}, {path}): {s}")
            pending[k] = (out_r, out_c, psw_r, psw_c)
        else:
            k = event[1]
            out_r, out_c, psw_r, psw_c = pending.pop(k)
            g = torch.Generator().manual_seed(900 + k)
            grad = torch.randn(out_r.shape, generator=g).to(dev)
            out_r.backward(grad)
            out_c.backward(grad)
            if psw_r is not None and psw_r.requires_grad:
                torch.testing.assert_close(
                    psw_c.grad, psw_r.grad, atol=1e-5, rtol=1e-5,
                    msg=lambda s: f"bwd({k}): per-sample-weight grad: {s}",
                )
    assert not pending
    torch.cuda.synchronize()
    for spec, wc, wr in zip(PAIR_SPECS, cached.split_embedding_weights(), ref.split_embedding_weights()):
        torch.testing.assert_close(
            wc, wr.cpu(), atol=1e-5, rtol=1e-4, msg=lambda s: f"table {spec[0]}: {s}"
        )
    torch.testing.assert_close(cached.momentum, ref.momentum.cpu(), atol=1e-6, rtol=0)
    return cached


@pytest.mark.gpu
class TestCoherence:
    @pytest.mark.parametrize("name", list(SCHEDULES))
    def test_schedule(self, name):
        cached = run_pair(SCHEDULES[name])
        assert not cached._prefetched, "a prefetch() entry was left behind"

    @pytest.mark.parametrize("order", ["inline", "pipeline"])
    @pytest.mark.parametrize("path", PATHS)
    def test_path(self, path, order):
        make = inline_order if order == "inline" else pipeline_order
        pooling = PoolingMode.MEAN if path == "mean" else PoolingMode.SUM
        run_pair(make(4, "sum" if path == "mean" else path), pooling)

    @pytest.mark.parametrize("order", ["inline", "pipeline"])
    @pytest.mark.parametrize("other", ["vbe8", "seq"])
    def test_mixed_paths(self, other, order):
        run_pair((MIXED if order == "inline" else MIXED_PIPELINED)[other])

    def test_forward_out_of_prefetch_order_raises(self):
        """The entry a forward consumes must be its own batch's (checked by length)."""
        cached, _ = make_cached(PAIR_SPECS)
        idx, off, _ = pair_batch(0)
        n0, short = PAIR_B * PAIR_L, (PAIR_B - 1) * PAIR_L  # the same batch, one bag fewer
        idx7 = np.concatenate([idx[:short], idx[n0 : n0 + short]])
        cached.prefetch(torch.from_numpy(idx7).cuda(), torch.from_numpy(off[: 2 * PAIR_B - 1]).cuda())
        with pytest.raises(RuntimeError, match="prefetch"):
            cached(torch.from_numpy(idx).cuda(), torch.from_numpy(off).cuda())


# ---------------------------------------------------------------------------
# D. batches of the pipeline test in test_gpu_e2e.py
# ---------------------------------------------------------------------------

PIPE_ROWS = (96, 64)
PIPE_B = 16


def pipeline_ids(k):
    """Batch k of the pipeline test: one id per sample and feature, 16 + 16 unique
    ids that fill the one-set cache, disjoint from the neighbouring batches."""
    g = np.random.default_rng(40 + k)
    return [g.permutation(PIPE_B) + (k % 4) * PIPE_B for _ in PIPE_ROWS]


class TestPreconditionsD:
    def test_each_prefetch_displaces_the_current_batch(self):
        m = LxuCacheModel(1, 64, _tables([(96, 64), (64, 64)], 0))
        lin = [np.concatenate([i0, i1 + PIPE_ROWS[0]]) for i0, i1 in map(pipeline_ids, range(4))]
        for i0, i1 in map(pipeline_ids, range(4)):
            assert i0.max() < 96 and i1.max() < 64
        m.populate(lin[0])
        for step in range(6):  # 4 batches, cycling
            ev = m.populate(lin[(step + 1) % 4])
            assert len(set(ev) & set(lin[step % 4].tolist())) >= 8, step
