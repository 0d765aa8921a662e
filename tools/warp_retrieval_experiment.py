#!/usr/bin/env python3
"""Does the warped metric find what the aligned and the shifted search miss?  A synthetic check in
float64 numpy, no GPU: 2000 random items of 4 x 32 cells over K = 64 codes with a random codebook's distance table as the
per-cell cost; a query is 24 columns of one item read along a random path -- start at column 4, steps 0 / 1 / 2, drift kept
within +-4 of the start -- with 20 % of its cells replaced by random codes.  Three searches, all by the specification's
float64 recurrence (tests/code_warp_search_spec.py):
  warped    the band (0, 8)
  shifted   the best of the nine straight alignments at offsets 0 .. 8 (closed bands (o, o)): the shifted search
  aligned   the straight alignment at the start offset 4 alone
and for each the number of queries whose source item is ranked first (ties by item index).  Synthetic codes, not sounds.

  python tools/warp_retrieval_experiment.py [--queries 400] [--items 2000] [--seed 0] [--merge-into profiles/code_search_warp.json]
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import code_warp_search_spec as WS  # noqa: E402

F, T, W, K, D, START, DRIFT, NOISE = 4, 32, 24, 64, 8, 4, 4, 0.2


def random_path(rng):
    """p(0) = START, steps in {0, 1, 2}, |p(i) - i - START| <= DRIFT."""
    path = [START]
    for i in range(1, W):
        steps = [s for s in (0, 1, 2) if abs(path[-1] + s - i - START) <= DRIFT]
        path.append(path[-1] + int(rng.choice(steps)))
    return np.array(path)


def run(queries, items, seed):
    rng = np.random.default_rng(seed)
    codebook = rng.standard_normal((K, D)).astype(np.float32).astype(np.float64)
    table = ((codebook[:, None, :] - codebook[None, :, :]) ** 2).sum(-1).astype(np.float32)
    codes = rng.integers(0, K, (items, F, T)).astype(np.uint16)
    first = {"warped": 0, "shifted": 0, "aligned": 0}
    for _ in range(queries):
        source = int(rng.integers(0, items))
        path = random_path(rng)
        assert WS.path_admissible(path, T, START - DRIFT, START + DRIFT)
        query = codes[source][:, path].copy()
        noisy = rng.random((F, W)) < NOISE
        query[noisy] = rng.integers(0, K, int(noisy.sum()))
        part = WS.Part(codes, table[query.reshape(1, -1).astype(np.int64)])
        cost = WS.column_cost([part], 0, np.float64)
        warped = WS.align(cost, START - DRIFT, START + DRIFT)[0]
        straight = np.stack([WS.align(cost, o, o)[0] for o in range(START - DRIFT, START + DRIFT + 1)])
        for name, dist in (("warped", warped), ("shifted", straight.min(0)), ("aligned", straight[DRIFT])):
            first[name] += int(np.argsort(dist, kind="stable")[0] == source)
    return {"what": "float64 numpy by tests/code_warp_search_spec.py; synthetic uniform codes, not sounds",
            "items": items, "queries": queries, "seed": seed, "F": F, "T": T, "W": W, "K": K,
            "query": f"{W} columns of an item along a random path from column {START}, steps 0/1/2, drift within +-{DRIFT}; "
                     f"{int(NOISE * 100)} % of the cells replaced",
            "source_ranked_first": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--merge-into", default=None, help="a JSON record to which the result is added as retrieval_experiment")
    args = ap.parse_args()
    res = run(args.queries, args.items, args.seed)
    print(json.dumps(res))
    if args.merge_into:
        path = pathlib.Path(args.merge_into)
        record = json.loads(path.read_text()) if path.exists() else {}
        record["retrieval_experiment"] = res
        path.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
