"""Driver-contract checks for bench.py output (@gpu)."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = [
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
]


@pytest.mark.gpu
def test_bench_json_contract(tmp_path):
    import numpy as np

    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--scale", "1e-4",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    for k in REQUIRED:
        assert k in res, f"missing field {k}"
    assert res["n_gpus"] == 1
    assert res["scaling"] == "weak"
    assert res["higher_is_better"] is True
    assert res["value"] > 0 and res["ms_per_step"] > 0
    assert "global_batch" in res["config"]
    assert res["steps"] == 3 and res["warmup"] == 1
    # --dump-outputs: what the last timed step returned, as float32 arrays
    assert sorted(f.name for f in tmp_path.iterdir()) == [
        "labels.npy", "logits.npy", "loss.npy",
    ]
    B = res["config"]["local_batch"]
    for name, shape in (("loss", (1,)), ("logits", (B,)), ("labels", (B,))):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape
        assert np.isfinite(a).all()
    assert set(np.unique(np.load(tmp_path / "labels.npy"))) <= {0.0, 1.0}


def test_bench_world2_gloo_cpu(tmp_path):
    """Rehearse the driver's multi-rank launch end-to-end on gloo/CPU:
    torch.distributed.run -> bench.py world 2 -> planner + DMP + pipeline +
    collectives + MAX-over-ranks JSON aggregation."""
    env = dict(os.environ, TREC_BENCH_CPU="1", MASTER_ADDR="127.0.0.1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=2", "--master-addr=127.0.0.1",
         "--master-port=29621", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--batch-size", "64", "--scale", "1e-4",
         "--full", "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=600, env=env, cwd=REPO,
    )
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2
    assert res["config"]["global_batch"] == 128
    # one set of dumped outputs per rank, each the local batch of 64
    import numpy as np

    for rank in (0, 1):
        logits = np.load(tmp_path / f"logits_rank{rank}.npy")
        assert logits.dtype == np.float32 and logits.shape == (64,)
        assert np.isfinite(np.load(tmp_path / f"loss_rank{rank}.npy")).all()


def test_bench_plan_world8_cpu():
    """The 8-GPU plan the driver's SCALE run will request must be buildable
    (no OOM/partition errors) — planner is pure CPU."""
    import bench
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
    from torchrec_amd.distributed.planner.types import Topology

    model = bench.build_model(1.0)
    for world in (2, 4, 8):
        planner = EmbeddingShardingPlanner(
            topology=Topology(
                world_size=world, compute_device="cuda", batch_size=8192
            )
        )
        sharder = EmbeddingBagCollectionSharder(
            fused_params={"optimizer": "rowwise_adagrad", "learning_rate": 0.01}
        )
        plan = planner.plan(model, [sharder])
        mplan = plan.get_plan_for_module("model.sparse_arch.ebc") or next(
            iter(plan.plan.values())
        )
        entries = dict(mplan.items()) if hasattr(mplan, "items") else dict(mplan)
        assert len(entries) == len(bench.DLRM_EMB_ROWS)
        for name, ps in entries.items():
            assert ps.compute_kernel in ("fused", "fused_uvm", "fused_uvm_caching")
