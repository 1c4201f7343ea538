"""How much the cubeful bearoff table's one approximation costs (DESIGN.md §15;
profiles/cube_bearoff/cap_approximation.json): the table assumes an unlimited cube, the rollout's
cube stops at 2^cap.  In numpy float64 at K = 3 over the oracle's successors, the unlimited table
is compared with the tables that allow at most j = 1..4 further doubles (j = 0 is the dead cube,
the cubeless 2 W - 1): per j the largest difference over all pairs and states.  No GPU.

    python tools/cube_bearoff_cap.py OUT.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mlp-ppo-2ply-p3_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def limited(succ, n, e_opp_after):
    """cube_table_reference with DT[a][b] = 2 e_opp_after[a][b]: the opponent's equity after a
    double comes from the table with one double fewer."""
    from bgx.bearoff import CUBE_CHILD, ROLLS21
    f = np.float64
    E = np.zeros((3, n, n), f)
    E[:, :, 0], E[:, 0, 1:] = -1, 1
    p = np.array([1 / 36 if a == b else 2 / 36 for a, b in ROLLS21], f)
    flat = [[np.asarray(s, np.int64) for s in succ[a]] for a in range(n)]
    depth = np.zeros(n, np.int64)
    for a in range(1, n):
        depth[a] = 1 + max(depth[int(x)] for s in flat[a] for x in s)
    by_depth = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]
    for t in range(2, 2 * len(by_depth) - 1):
        for a in range(1, n):
            db = t - int(depth[a])
            if not 1 <= db < len(by_depth):
                continue
            bs = by_depth[db]
            acc = np.zeros((3, len(bs)), f)
            for r in range(21):
                s = flat[a][r]
                for st in range(3):
                    acc[st] += p[r] * np.where(s == 0, 1.0, -E[CUBE_CHILD[st]][np.ix_(bs, s)]).max(axis=1)
            cash = np.minimum(2 * e_opp_after[a, bs], 1)
            E[0, a, bs], E[1, a, bs], E[2, a, bs] = np.maximum(acc[0], cash), np.maximum(acc[1], cash), acc[2]
    return E


def main():
    import cube_bearoff_ref as CR
    K = 3
    succ, n = CR.oracle_succ(K), len(CR.ordered_configs(K))
    W, E, _ = CR.references(K, "float64")
    prev = np.broadcast_to(2 * W - 1, (3, n, n))                # j = 0: the dead cube
    rows = [dict(further_doubles=0, max_abs_difference=float(np.abs(prev - E)[:, 1:, 1:].max()))]
    for j in range(1, 5):
        cur = limited(succ, n, prev[2])
        rows.append(dict(further_doubles=j, max_abs_difference=float(np.abs(cur - E)[:, 1:, 1:].max())))
        prev = cur
    doc = dict(K=K, dtype="float64", what="max over pairs and the three states of |E limited to j further doubles - E unlimited|",
               rows=rows)
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
