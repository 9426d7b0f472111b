"""Cases, float64 oracle and parent-pin generator for test_tbe_forward_tiles.

The pooled forward is driven through the raw op, so that every buffer the
kernel reads is laid out by the test. A case is a plain dict of numpy arrays.

Run as a script to (re)write the parent pins:

    python -m tests.tbe_forward_tiles_cases tests/golden/tbe_forward_tiles

That must be done on the GPU from the commit whose accumulation order is to be
pinned (the pins in the tree come from the last commit with the one-bag-per-slot
forward). Each pin stores inputs and output as raw bits, so the test depends on
no random generator.
"""

import os
import sys

import numpy as np
import torch

ROWS = 12  # rows per table; the last one is the poison row
POISON_ROW = ROWS - 1
POISON = 4096.0  # what an over-read row contributes
POISON_W = 64.0  # what an over-read per-sample weight multiplies by

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
OUT_CODE = {"fp32": 0, "bf16": 1, "fp16": 2}

# lengths below, at and past a flight (4) and an offsets / indices round
# (16, 32 or 64 lanes per slot)
LENGTHS = [0, 1, 3, 4, 5, 31, 32, 33, 70]
LENGTHS_POW2 = [0, 1, 2, 4, 8, 32, 64]


def mixed_lengths(rng, n, menu):
    """n bag lengths: every entry of the menu (while n allows), shuffled, so
    that one tile of consecutive bags holds a mix."""
    reps = [menu[i % len(menu)] for i in range(n)]
    return rng.permutation(np.asarray(reps, dtype=np.int64))


def make_case(
    seed,
    dims,
    feat_table,
    B,
    lengths,
    tdtype="fp32",
    odtype="fp32",
    psw=False,
    mean=False,
    cached=False,
    dyadic=True,
    mag=8,
):
    """lengths: [F * B] feature-major. dyadic weights are integers in
    [-mag, mag] / 8 and psw in {0.5, 1, 2}: every partial sum is exact."""
    rng = np.random.default_rng(seed)
    F = len(feat_table)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.shape == (F * B,)
    tables = []
    for d in dims:
        if dyadic:
            w = rng.integers(-mag, mag + 1, size=(ROWS, d)).astype(np.float32) / 8.0
        else:
            w = rng.standard_normal((ROWS, d)).astype(np.float32)
        w[POISON_ROW] = POISON
        tables.append(w)
    offsets = np.zeros(F * B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lengths)
    N = int(offsets[-1])
    indices = rng.integers(0, POISON_ROW, size=N).astype(np.int64)
    if psw:
        pw = (
            rng.choice(np.asarray([0.5, 1.0, 2.0], dtype=np.float32), size=N)
            if dyadic
            else rng.uniform(0.25, 2.0, size=N).astype(np.float32)
        )
    else:
        pw = None
    case = dict(
        dims=list(dims),
        feat_table=list(feat_table),
        B=int(B),
        tables=tables,
        indices=indices,
        offsets=offsets,
        psw=pw,
        mean=bool(mean),
        tdtype=tdtype,
        odtype=odtype,
        cache_weights=None,
        cache_loc=None,
    )
    if cached:
        max_D = max(dims)
        slots = 24
        if dyadic:
            cw = rng.integers(-mag, mag + 1, size=(slots, max_D)).astype(np.float32) / 8.0
        else:
            cw = rng.standard_normal((slots, max_D)).astype(np.float32)
        # about half of the positions hit, in no pattern: hits and misses
        # share a flight
        loc = rng.integers(0, slots, size=N).astype(np.int32)
        loc[rng.random(N) < 0.5] = -1
        case["cache_weights"], case["cache_loc"] = cw, loc
    return case


def table_values(case):
    """The tables as the kernel sees them: rounded to the table dtype."""
    dt = TORCH_DT[case["tdtype"]]
    return [torch.from_numpy(w).to(dt).to(torch.float64).numpy() for w in case["tables"]]


def oracle64(case, mutant=None):
    """float64 gather-and-sum; mean divides by the bag length in float64.
    mutant in {None, 'drop_last', 'neighbour', 'no_psw'} breaks it on purpose."""
    dims, ft, B = case["dims"], case["feat_table"], case["B"]
    tabs = table_values(case)
    off, idx, pw = case["offsets"], case["indices"], case["psw"]
    loc, cw = case["cache_loc"], case["cache_weights"]
    total_D = sum(dims[t] for t in ft)
    out = np.zeros((B, total_D), dtype=np.float64)
    col = 0
    for f, t in enumerate(ft):
        D = dims[t]
        for b in range(B):
            i0, i1 = int(off[f * B + b]), int(off[f * B + b + 1])
            pos = list(range(i0, i1))
            if mutant == "drop_last" and pos:
                pos = pos[:-1]
            if mutant == "neighbour" and i1 < len(idx):
                pos = pos + [i1]
            acc = np.zeros(D, dtype=np.float64)
            for i in pos:
                if loc is not None and loc[i] >= 0:
                    row = cw[loc[i], :D].astype(np.float64)
                else:
                    row = tabs[t][idx[i]]
                w = 1.0 if (pw is None or mutant == "no_psw") else float(pw[i])
                acc += w * row
            if case["mean"] and i1 > i0:
                acc /= float(i1 - i0)
            out[b, col : col + D] = acc
        col += D
    return out


def sequential32(case):
    """The kernel's arithmetic on the CPU: fp32 sum in ascending position
    order from zero, then * fl32(1 / len) for mean. No fused multiply-add:
    on dyadic inputs the product is exact, so it makes no difference."""
    dims, ft, B = case["dims"], case["feat_table"], case["B"]
    tabs = [w.astype(np.float32) for w in table_values(case)]
    off, idx, pw = case["offsets"], case["indices"], case["psw"]
    loc, cw = case["cache_loc"], case["cache_weights"]
    total_D = sum(dims[t] for t in ft)
    out = np.zeros((B, total_D), dtype=np.float32)
    col = 0
    for f, t in enumerate(ft):
        D = dims[t]
        for b in range(B):
            i0, i1 = int(off[f * B + b]), int(off[f * B + b + 1])
            acc = np.zeros(D, dtype=np.float32)
            for i in range(i0, i1):
                row = cw[loc[i], :D] if (loc is not None and loc[i] >= 0) else tabs[t][idx[i]]
                w = np.float32(1.0) if pw is None else np.float32(pw[i])
                acc = acc + w * row
            if case["mean"] and i1 > i0:
                acc = acc * (np.float32(1.0) / np.float32(i1 - i0))
            out[b, col : col + D] = acc
        col += D
    return out


def run_forward(case, device, embed=False):
    """The op's output for a case. embed=True passes indices, offsets, psw and
    cache_loc as views into the middle of larger buffers whose surroundings
    hold valid values that point at the poison row / weight."""
    import torchrec_amd.ops as ops

    assert ops.extension_available()  # loads the library behind torch.ops.trec_amd

    dims, ft, B = case["dims"], case["feat_table"], case["B"]
    dt = TORCH_DT[case["tdtype"]]
    weights = torch.cat([torch.from_numpy(w).reshape(-1) for w in case["tables"]]).to(dt)
    elem = np.zeros(len(dims), dtype=np.int64)
    elem[1:] = np.cumsum([w.size for w in case["tables"]])[:-1]
    d_out = np.zeros(len(ft) + 1, dtype=np.int64)
    d_out[1:] = np.cumsum([dims[t] for t in ft])
    pad = 96 if embed else 0

    def mid(a, fill):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not embed:
            return t.to(device)
        buf = torch.full((pad + t.numel() + pad,), fill, dtype=t.dtype)
        buf[pad : pad + t.numel()] = t
        return buf.to(device)[pad : pad + t.numel()]

    N = case["indices"].size
    indices = mid(case["indices"], POISON_ROW)
    # a stray offset is a valid one too: the end of the indices
    offsets = mid(case["offsets"], N)
    psw = (
        mid(case["psw"], POISON_W)
        if case["psw"] is not None
        else torch.empty(0, dtype=torch.float32, device=device)
    )
    if case["cache_loc"] is not None:
        cache_w = torch.from_numpy(case["cache_weights"]).to(device)
        cache_loc = mid(case["cache_loc"], -1)
    else:
        cache_w = torch.empty(0, dtype=torch.float32, device=device)
        cache_loc = torch.empty(0, dtype=torch.int32, device=device)
    out = torch.ops.trec_amd.tbe_forward_pooled(
        weights.to(device),
        torch.from_numpy(elem).to(device),
        torch.tensor(dims, dtype=torch.int32, device=device),
        torch.tensor(ft, dtype=torch.int32, device=device),
        torch.from_numpy(d_out).to(device),
        indices,
        offsets,
        psw,
        B,
        int(d_out[-1]),
        max(dims),
        case["mean"],
        cache_w,
        cache_loc,
        OUT_CODE[case["odtype"]],
    )
    torch.cuda.synchronize()
    return out.cpu()


# ---------------------------------------------------------------------------
# parent pins: arbitrary real-valued weights, so the order of the adds shows
# ---------------------------------------------------------------------------


def pin_cases():
    def lens(seed, n, menu=LENGTHS):
        return mixed_lengths(np.random.default_rng(seed), n, menu)

    B = 9  # one tile holding every length of the menu, per feature
    return {
        "mixed_d_sum": make_case(
            11, [4, 64, 128], [0, 1, 2, 1], B, lens(1, 4 * B), dyadic=False
        ),
        "psw_sum": make_case(12, [64, 128], [0, 1, 1], B, lens(2, 3 * B), psw=True, dyadic=False),
        "mean": make_case(13, [64, 128], [0, 1, 0], B, lens(3, 3 * B), mean=True, dyadic=False),
        "bf16_tables_fp32_out": make_case(
            14, [4, 128], [0, 1, 1], B, lens(4, 3 * B), tdtype="bf16", psw=True, dyadic=False
        ),
        "fp32_tables_bf16_out": make_case(
            15, [128, 128], [0, 1, 0], B, lens(5, 3 * B), odtype="bf16", dyadic=False
        ),
        "cached": make_case(
            16, [64, 128], [0, 1, 1], B, lens(6, 3 * B), psw=True, cached=True, dyadic=False
        ),
        "d256_fp16_mean_psw": make_case(
            17, [256], [0, 0], B, lens(7, 2 * B), tdtype="fp16", odtype="fp16", psw=True,
            mean=True, dyadic=False,
        ),
    }


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def save_pin(path, case, out):
    arrays = {f"table{i}": w for i, w in enumerate(case["tables"])}
    for k in ("indices", "offsets", "psw", "cache_weights", "cache_loc"):
        if case[k] is not None:
            arrays[k] = case[k]
    arrays["dims"] = np.asarray(case["dims"], dtype=np.int64)
    arrays["feat_table"] = np.asarray(case["feat_table"], dtype=np.int64)
    arrays["meta"] = np.asarray(
        [case["B"], int(case["mean"]), OUT_CODE[case["tdtype"]], OUT_CODE[case["odtype"]]],
        dtype=np.int64,
    )
    arrays["out_bits"] = _bits(out)
    np.savez_compressed(path, **arrays)


def load_pin(path):
    z = np.load(path)
    names = {v: k for k, v in OUT_CODE.items()}
    dims = [int(d) for d in z["dims"]]
    B, mean, tcode, ocode = (int(v) for v in z["meta"])
    case = dict(
        dims=dims,
        feat_table=[int(t) for t in z["feat_table"]],
        B=B,
        tables=[z[f"table{i}"] for i in range(len(dims))],
        indices=z["indices"],
        offsets=z["offsets"],
        psw=z["psw"] if "psw" in z else None,
        mean=bool(mean),
        tdtype=names[tcode],
        odtype=names[ocode],
        cache_weights=z["cache_weights"] if "cache_weights" in z else None,
        cache_loc=z["cache_loc"] if "cache_loc" in z else None,
    )
    return case, z["out_bits"]


def main(out_dir):
    import torchrec_amd.ops as ops

    assert ops.extension_available() and torch.cuda.is_available()
    os.makedirs(out_dir, exist_ok=True)
    for name, case in pin_cases().items():
        out = run_forward(case, "cuda")
        path = os.path.join(out_dir, name + ".npz")
        save_pin(path, case, out)
        print(name, tuple(out.shape), out.dtype, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
