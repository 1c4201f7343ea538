"""Ground truth for the bearoff tests: lane records built from configurations and the oracle's
movegen / apply_move on them -- an enumeration independent of csrc/bg_bearoff.h."""
import numpy as np

import oracle as O

ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]


def all_configs(K):
    """Every six-count tuple (distances 1..6) with a sum of at most K."""
    out = []

    def rec(prefix, left):
        if len(prefix) == 6:
            out.append(tuple(prefix))
            return
        for v in range(left + 1):
            rec(prefix + [v], left - v)
    rec([], K)
    return out


def record(c1, c2, mover, roll=(0, 0)):
    """uint8[64]: PLAYER1 with configuration c1 (distance d on point 24 - d), PLAYER2 with c2
    (distance d on point d - 1), the rest of each side's 15 checkers off."""
    r = np.zeros(64, np.uint8)
    for d in range(1, 7):
        r[24 - d] = c1[d - 1]
        r[24 + d - 1] = c2[d - 1]
    r[50], r[51] = 15 - sum(c1), 15 - sum(c2)
    r[52] = mover
    r[53], r[54] = roll
    return r


def config_of(board52, player):
    b = np.asarray(board52)
    return tuple(int(b[24 - d]) if player == 0 else int(b[24 + d - 1]) for d in range(1, 7))


def oracle_successors(c, mover=0, opp=(1, 0, 0, 0, 0, 0)):
    """The 21 sets of configurations `mover` reaches from c with a legal play of each roll
    (c itself when the roll cannot be played), against the opponent configuration `opp`."""
    rec = record(c, opp, 0) if mover == 0 else record(opp, c, 1)
    board = rec[:52].view(np.int8)
    out = []
    for roll in ROLLS21:
        moves, n = O.movegen(board, mover, roll)
        if n == 0:
            out.append({tuple(c)})
        else:
            out.append({config_of(O.apply_move(board, mover, int(m)), mover) for m in moves})
    return out
