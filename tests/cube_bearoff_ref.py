"""Shared ground truth of the cubeful bearoff tests: the table's index order, the oracle's
successor sets as index lists, and the host references computed once per K."""
import functools

import numpy as np

import bearoff_ref as BR


@functools.lru_cache(maxsize=None)
def ordered_configs(K):
    """The configurations of at most K checkers in the table's order: (pip count, base-9 key)."""
    def key(c):
        return (sum((d + 1) * v for d, v in enumerate(c)), sum(v * 9 ** d for d, v in enumerate(c)))
    return tuple(sorted(BR.all_configs(K), key=key))


@functools.lru_cache(maxsize=None)
def oracle_succ(K):
    """succ[a][r] = the sorted index list of the oracle's successor set (its own movegen)."""
    cfg = ordered_configs(K)
    index = {c: i for i, c in enumerate(cfg)}
    return [[sorted(index[s] for s in sets) for sets in BR.oracle_successors(c)] for c in cfg]


@functools.lru_cache(maxsize=None)
def references(K, dtype_name):
    """(W, equity[3], nd[2]) by bgx.bearoff's host recurrences over the oracle's successors.
    Shared between tests: do not write to them."""
    from bgx.bearoff import cube_table_reference, table_reference
    dtype = {"float32": np.float32, "float64": np.float64}[dtype_name]
    succ, n = oracle_succ(K), len(ordered_configs(K))
    W = table_reference(succ, n, dtype)
    E, ND = cube_table_reference(succ, n, dtype)
    for x in (W, E, ND):
        x.setflags(write=False)
    return W, E, ND


def records_of(K, pairs, movers):
    """uint8[len, 64]: pair (a, b) of table indices with `mover` on roll holding a (the mover's
    configuration is a, the opponent's b)."""
    cfg = ordered_configs(K)
    out = []
    for (a, b), m in zip(pairs, movers):
        out.append(BR.record(cfg[a], cfg[b], 0) if m == 0 else BR.record(cfg[b], cfg[a], 1))
    return np.stack(out)
