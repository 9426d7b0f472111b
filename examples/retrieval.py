"""Two-tower retrieval: train a few steps, index every item, query the index.

    python examples/retrieval.py [--items 5000 --users 1000 --k 10 --metric ip
                                  --num_centroids 64 --num_probe 8]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchrec_amd.models import (  # noqa: E402
    TwoTower,
    TwoTowerRetrieval,
    TwoTowerTrain,
    build_candidate_index,
)
from torchrec_amd.modules import (  # noqa: E402
    EmbeddingBagCollection,
    EmbeddingBagConfig,
    FlatIndex,
    IVFFlatIndex,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor  # noqa: E402


def _one_id_per_row(keys, ids):
    return KeyedJaggedTensor(keys=keys, values=torch.cat(ids),
                             lengths=torch.ones_like(torch.cat(ids)), stride=ids[0].numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=5000)
    ap.add_argument("--users", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", choices=["ip", "l2"], default="ip")
    ap.add_argument("--num_centroids", type=int, default=0,
                    help="lists of an IVF index; 0 searches exhaustively")
    ap.add_argument("--num_probe", type=int, default=8, help="lists searched per query")
    args = ap.parse_args()
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    torch.manual_seed(0)

    tables = [
        EmbeddingBagConfig(num_embeddings=n, embedding_dim=64, name=f"t_{f}", feature_names=[f])
        for f, n in (("user", args.users), ("item", args.items))
    ]
    two_tower = TwoTower(EmbeddingBagCollection(tables=tables, device=device),
                         ["user"], ["item"], [128, 64], device=device)
    train = TwoTowerTrain(two_tower)
    opt = torch.optim.Adam(train.parameters(), lr=1e-2)
    for step in range(args.steps):
        users = torch.randint(0, args.users, (256,), device=device)
        items = (users * 7 + 3) % args.items  # a learnable user -> item rule
        loss = train(_one_id_per_row(["user", "item"], [users, items]))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"trained {args.steps} steps, loss {loss.item():.3f}")

    all_items = torch.arange(args.items, device=device)
    if args.num_centroids:
        index = IVFFlatIndex(64, args.num_centroids, nprobe=args.num_probe, metric=args.metric,
                             device=device)
    else:
        index = FlatIndex(64, metric=args.metric, device=device)
    index = build_candidate_index(
        two_tower, (_one_id_per_row(["item"], [b]) for b in all_items.split(1024)), index)
    print(f"indexed {len(index)} items in a {type(index).__name__}")

    model = TwoTowerRetrieval.from_two_tower(two_tower, index, args.k)
    users = torch.arange(4, device=device)
    with torch.no_grad():
        logits, ids = model(_one_id_per_row(["user"], [users]))
    for u, i, s in zip(users.tolist(), ids.tolist(), logits.tolist()):
        print(f"user {u}: items {i[:5]} ... logits {[round(x, 3) for x in s[:5]]}")


if __name__ == "__main__":
    main()
