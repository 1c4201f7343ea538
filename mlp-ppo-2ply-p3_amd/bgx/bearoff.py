"""Exact two-sided bearoff database (the device side is csrc/bg_bearoff.h behind
bgx_bearoff_* of include/bgx.h).  Once both sides have at most K checkers left, all in their
home boards, the cubeless game is a race between two independent six-point configurations, and
W[a][b] -- the probability that the side on roll with configuration a wins against b under
perfect play -- is a finite dynamic program.  The table gives

  * the true value of endgame positions (BearoffDB.lookup; equity in points = 2 W - 1),
  * a perfect endgame player (BearoffPlayer: one table read per legal move),
  * an exact truncation for rollouts (Rollout.run(..., bearoff=db), bgx/rollout.py).

A configuration is the six counts c[d-1], d = 1..6, of checkers at distance d from bearing off
(PLAYER1: point 24 - d; PLAYER2: point d - 1).  BearoffDB.configs() publishes the index order.

The table stops at 8 checkers a side.  OneSidedBearoffDB (csrc/bg_bearoff1.h
behind bgx_bearoff1_*) covers every pure home-board race, up to all 15 checkers: per
configuration the distribution of the number of rolls to bear off, and from two rows an
approximate win probability (each side minimises its own mean number of rolls), with
OneSidedPlayer and the same rollout cut.  Because the cut's values are then approximate, the
`equity_stderr` of a rollout cut at this table measures the spread of the sample and no longer
the error against the truth.

CubefulBearoffDB (csrc/bg_bearoff_cube.h behind bgx_bearoff_cube_*) adds the doubling
cube to the exact table: the money-play equity of every race in it with the cube centred, owned
and the opponent's, the exact answer to "double or not, take or pass?" (lookup), and the cut of
cubeful rollouts (Rollout.run(..., cube=rule, cube_bearoff=cdb)).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check
from .engine import R_CUR, R_OVER, _ptr, _stream

MAX_CHECKERS = 8
MAX_CHECKERS1 = 15                  # the one-sided table
ROW = 32                            # entries of a one-sided row: t = 0..31 rolls
# the 21 rolls in bgx_two_ply's order and their probabilities as the table's build adds them
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]
ROLL_P = np.array([1.0 / 36.0 if a == b else 2.0 / 36.0 for a, b in ROLLS21], np.float32)


class BearoffDB:
    """The table for at most `max_checkers` (1..8) checkers a side, built on `device` on the
    current stream; n = C(max_checkers + 6, 6) configurations (924 at the default 6)."""

    kind = "two-sided"
    lookup_entry = "bgx_bearoff_lookup"            # the C entry points of this kind of table
    cut_entry = "bgx_rollout_bearoff_cut"          # (BearoffPlayer; Rollout.run_lanes)

    def __init__(self, max_checkers: int = 6, device=None):
        K = int(max_checkers)
        if not 1 <= K <= MAX_CHECKERS:
            raise ValueError(f"BearoffDB: max_checkers must be in 1..{MAX_CHECKERS}, got {max_checkers}")
        self._lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise ValueError("BearoffDB needs a GPU device (HIP); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        h = ctypes.c_void_p()
        check(self._lib.bgx_bearoff_create(dev.index, K, _stream(dev), ctypes.byref(h)), "bgx_bearoff_create")
        self._h = h
        b = _lib.BgxBearoffBuffers()
        check(self._lib.bgx_bearoff_buffers_get(h, ctypes.byref(b)), "bgx_bearoff_buffers_get")
        self.n, self.K = int(b.n), int(b.max_checkers)
        # copies of the small tables; the big one stays where it is (table())
        m = self.n * 21
        self._succ_off = self._view(b.succ_off, (m + 1,), torch.int32).cpu().numpy()
        self._succ = self._view(b.succ, (int(self._succ_off[-1]),), torch.int32).cpu().numpy()
        self._configs = self._view(b.configs, (self.n, 6), torch.int8)
        self._table = self._view(b.table, (self.n, self.n), torch.float32)
        self._index = {tuple(int(v) for v in c): i for i, c in enumerate(self._configs.cpu().numpy())}

    def _view(self, ptr, shape, dtype):
        """A tensor over the database's own device memory (alive as long as this object)."""
        n = int(np.prod(shape))
        size = n * torch.empty(0, dtype=dtype).element_size()
        iface = {"shape": (size,), "typestr": "|u1", "data": (int(ptr), False), "version": 3, "strides": None}
        holder = type("_DevMem", (), {"__cuda_array_interface__": iface, "_owner": self})()
        t = torch.as_tensor(holder, device=self.device)
        return t.view(dtype).view(*shape)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.bgx_bearoff_destroy(h)
            except Exception:
                pass
            self._h = None

    def handle(self):
        return self._h

    def table(self) -> torch.Tensor:
        """W as an [n, n] fp32 tensor view of the database's memory (do not write to it)."""
        return self._table

    def configs(self) -> torch.Tensor:
        """The index order: [n, 6] int8, row i = the counts of configuration i at distances 1..6."""
        return self._configs

    def successors(self, idx: int) -> list:
        """The 21 sorted lists (one per roll, ROLLS21's order) of the configurations that
        configuration `idx` reaches with a legal play of the roll."""
        i = int(idx)
        if not 0 <= i < self.n:
            raise IndexError(f"successors: configuration index {idx} not in [0, {self.n})")
        off = self._succ_off[21 * i:21 * i + 22]
        return [self._succ[off[r]:off[r + 1]].tolist() for r in range(21)]

    def index_of(self, config) -> int:
        """The index of a configuration given as its six counts (a host convenience)."""
        key = tuple(int(v) for v in config)
        if len(key) != 6 or key not in self._index:
            raise ValueError(f"index_of: {config!r} is not six counts with a sum of at most {self.K}")
        return self._index[key]

    def lookup(self, records: torch.Tensor, out=None):
        """(in_db uint8[n], win f32[n]) for uint8 [n, 64] lane records on the database's device:
        in_db = the record is in the table (bgx_bearoff_lookup's test), win = the mover's exact
        win probability before its roll -- written only where in_db is 1; the other entries
        keep what `out` = (in_db, win) held (NaN without `out`)."""
        r = records
        if r.dim() != 2 or r.shape[1] != 64 or r.dtype != torch.uint8 or r.device != self.device:
            raise ValueError(f"lookup: records must be uint8 [n, 64] on {self.device}, got {r.dtype} "
                             f"{tuple(r.shape)} on {r.device}")
        r = r.contiguous()
        n = r.shape[0]
        if out is None:
            out = (torch.empty(n, dtype=torch.uint8, device=self.device),
                   torch.full((n,), float("nan"), dtype=torch.float32, device=self.device))
        in_db, win = out
        check(self._lib.bgx_bearoff_lookup(self._h, _ptr(r), n, _ptr(in_db), _ptr(win), _stream(self.device)),
              "bgx_bearoff_lookup")
        return in_db, win

    def act(self, eng, sel, act: torch.Tensor, in_db=None):
        """bgx_bearoff_act: act[i] = the perfect move of every lane with sel[i] != 0 (None:
        every lane) whose record is in the table; the other entries stay."""
        check(self._lib.bgx_bearoff_act(eng._h, self._h, _ptr(sel), _ptr(act), _ptr(in_db), _stream(eng.device)),
              "bgx_bearoff_act")
        return act


class BearoffPlayer:
    """An arena player: the table's perfect move where the position is in the table, `inner`'s
    move elsewhere.  `inner` acts on sel & ~in_db only, so a 2-ply player does no search where
    the answer is known."""

    def __init__(self, inner, db: BearoffDB):
        self.inner, self.db = inner, db
        self.sync_free = bool(getattr(inner, "sync_free", False))
        self.buf = None

    def act(self, eng, sel, step):
        B, dev = eng.batch, eng.device
        if self.buf is None or self.buf[0].numel() != B or self.buf[0].device != dev:
            self.buf = (torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev),
                        torch.empty(B, dtype=torch.int32, device=dev))
        in_db, rest, act = self.buf
        check(getattr(self.db._lib, self.db.lookup_entry)(self.db._h, ctypes.c_void_p(eng.lanes_ptr()), B, _ptr(in_db),
                                                          None, _stream(dev)), self.db.lookup_entry)
        torch.logical_and(sel != 0, in_db == 0, out=rest.view(torch.bool))
        act.copy_(self.inner.act(eng, rest, step))
        return self.db.act(eng, sel, act)


class OneSidedBearoffDB:
    """The one-sided table (csrc/bg_bearoff1.h behind bgx_bearoff1_*) for at
    most `max_checkers` (1..15) checkers a side, built on `device` on the current stream:
    for each of the n = C(max_checkers + 6, 6) configurations (54,264 at the default 15) the
    distribution of the number of rolls it needs to bear off when it minimises their mean.
    Two rows give a race's win probability -- an approximation where BearoffDB is exact, but
    for every pure home-board race.  Configurations are indexed as in BearoffDB."""

    kind = "one-sided"
    lookup_entry = "bgx_bearoff1_lookup"
    cut_entry = "bgx_rollout_bearoff1_cut"
    _view = BearoffDB._view

    def __init__(self, max_checkers: int = MAX_CHECKERS1, device=None):
        K = int(max_checkers)
        if not 1 <= K <= MAX_CHECKERS1:
            raise ValueError(f"OneSidedBearoffDB: max_checkers must be in 1..{MAX_CHECKERS1}, got {max_checkers}")
        self._lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise ValueError("OneSidedBearoffDB needs a GPU device (HIP); there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        h = ctypes.c_void_p()
        check(self._lib.bgx_bearoff1_create(dev.index, K, _stream(dev), ctypes.byref(h)), "bgx_bearoff1_create")
        self._h = h
        b = _lib.BgxBearoff1Buffers()
        check(self._lib.bgx_bearoff1_buffers_get(h, ctypes.byref(b)), "bgx_bearoff1_buffers_get")
        self.n, self.K = int(b.n), int(b.max_checkers)
        self._dist = self._view(b.dist, (self.n, ROW), torch.float32)
        self._surv = self._view(b.surv, (self.n, ROW), torch.float32)
        self._mean = self._view(b.mean, (self.n,), torch.float32)
        self._choice = self._view(b.choice, (self.n, 21), torch.int32)
        self._configs = self._view(b.configs, (self.n, 6), torch.int8)
        self._index = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.bgx_bearoff1_destroy(h)
            except Exception:
                pass
            self._h = None

    def handle(self):
        return self._h

    def dist(self) -> torch.Tensor:
        """D as an [n, 32] fp32 view of the database's memory (do not write to it): D[a, t] =
        the probability that configuration a is borne off with exactly t rolls."""
        return self._dist

    def surv(self) -> torch.Tensor:
        """S as an [n, 32] fp32 view: S[a, t] = the probability that a needs at least t rolls."""
        return self._surv

    def mean(self) -> torch.Tensor:
        """The mean number of rolls, an [n] fp32 view."""
        return self._mean

    def choice(self) -> torch.Tensor:
        """[n, 21] int32 view: the configuration the table plays to from a with roll r (ROLLS21)."""
        return self._choice

    def configs(self) -> torch.Tensor:
        """The index order: [n, 6] int8, row i = the counts of configuration i at distances 1..6."""
        return self._configs

    def index_of(self, config) -> int:
        """The index of a configuration given as its six counts (a host convenience)."""
        if self._index is None:
            self._index = {tuple(int(v) for v in c): i for i, c in enumerate(self._configs.cpu().numpy())}
        key = tuple(int(v) for v in config)
        if len(key) != 6 or key not in self._index:
            raise ValueError(f"index_of: {config!r} is not six counts with a sum of at most {self.K}")
        return self._index[key]

    def lookup(self, records: torch.Tensor, out=None):
        """(in_db uint8[n], win f32[n]) for uint8 [n, 64] lane records on the database's device
        (bgx_bearoff1_lookup): in_db = 1 in the table with checkers of both sides off (equity
        2 win - 1), 2 in the table with all 15 checkers of a side on the board (win is the win
        probability, gammons are possible), 0 not in it.  win is written only where in_db is not
        0; the other entries keep what `out` = (in_db, win) held (NaN without `out`)."""
        r = records
        if r.dim() != 2 or r.shape[1] != 64 or r.dtype != torch.uint8 or r.device != self.device:
            raise ValueError(f"lookup: records must be uint8 [n, 64] on {self.device}, got {r.dtype} "
                             f"{tuple(r.shape)} on {r.device}")
        r = r.contiguous()
        n = r.shape[0]
        if out is None:
            out = (torch.empty(n, dtype=torch.uint8, device=self.device),
                   torch.full((n,), float("nan"), dtype=torch.float32, device=self.device))
        in_db, win = out
        check(self._lib.bgx_bearoff1_lookup(self._h, _ptr(r), n, _ptr(in_db), _ptr(win), _stream(self.device)),
              "bgx_bearoff1_lookup")
        return in_db, win

    def act(self, eng, sel, act: torch.Tensor, in_db=None):
        """bgx_bearoff1_act: act[i] = the move with the best win probability by the table, of
        every lane with sel[i] != 0 (None: every lane) whose record is in the table; the other
        entries stay."""
        check(self._lib.bgx_bearoff1_act(eng._h, self._h, _ptr(sel), _ptr(act), _ptr(in_db), _stream(eng.device)),
              "bgx_bearoff1_act")
        return act


class OneSidedPlayer(BearoffPlayer):
    """BearoffPlayer on a OneSidedBearoffDB: the table's move in every pure home-board race,
    `inner`'s move elsewhere.  It nests: BearoffPlayer(OneSidedPlayer(inner, db1), db) plays
    exactly where the small exact table reaches and by the one-sided table in the rest of the
    bearoff."""


class CubefulBearoffDB:
    """The cubeful exact table (csrc/bg_bearoff_cube.h behind bgx_bearoff_cube_*)
    over an existing BearoffDB `db`, built on db's device on the current stream: for every pair
    of its configurations the money-play equity of the side on roll in units of the current
    cube, for the cube centred, its own and the opponent's (unlimited cube, no gammons).  It
    answers "double or not, take or pass?" exactly for every position in the table (lookup) and
    cuts cubeful rollouts there (Rollout.run(..., cube=rule, cube_bearoff=cdb)).  The object
    keeps `db`, whose memory it reads."""

    kind = "cubeful"
    STATES = ("cen", "own", "opp")                 # the planes' order; nd has the first two
    _view = BearoffDB._view

    def __init__(self, db: BearoffDB):
        if not isinstance(db, BearoffDB):
            raise ValueError("CubefulBearoffDB: db must be a bearoff.BearoffDB")
        self._lib, self.db, self.device = db._lib, db, db.device
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._lib.bgx_bearoff_cube_create(db.handle(), _stream(self.device), ctypes.byref(h)),
                  "bgx_bearoff_cube_create")
        self._h = h
        b = _lib.BgxBearoffCubeBuffers()
        check(self._lib.bgx_bearoff_cube_buffers_get(h, ctypes.byref(b)), "bgx_bearoff_cube_buffers_get")
        self.n, self.K = int(b.n), int(b.max_checkers)
        self._equity = self._view(b.equity, (3, self.n, self.n), torch.float32)
        self._nd = self._view(b.nd, (2, self.n, self.n), torch.float32)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.bgx_bearoff_cube_destroy(h)
            except Exception:
                pass
            self._h = None

    def handle(self):
        return self._h

    def equity(self) -> torch.Tensor:
        """E as a [3, n, n] fp32 view of the table's memory (do not write to it): plane s, row a,
        column b = the equity of the side on roll with a against b in cube state STATES[s]."""
        return self._equity

    def nd(self) -> torch.Tensor:
        """ND as a [2, n, n] fp32 view: the same without a double now, for cen and own."""
        return self._nd

    def configs(self) -> torch.Tensor:
        """The index order, the cubeless database's."""
        return self.db.configs()

    def index_of(self, config) -> int:
        return self.db.index_of(config)

    def lookup(self, records: torch.Tensor, cube=None, cap: int = 6, out=None):
        """(in_db uint8[n], values f32[n, 4], flags uint8[n]) for uint8 [n, 64] lane records on
        the table's device (bgx_bearoff_cube_lookup): values = (nd, DT, e, cubeless 2 W - 1) of
        the record's mover holding the cube byte cube[i] (uint8[n], cube.pack(k, owner); None:
        centred at 1), written only where in_db is 1 (NaN elsewhere without `out`); flags bit 0:
        the mover may double, 1: it doubles, 2: the opponent takes, 3: the cube is dead."""
        r = records
        if r.dim() != 2 or r.shape[1] != 64 or r.dtype != torch.uint8 or r.device != self.device:
            raise ValueError(f"lookup: records must be uint8 [n, 64] on {self.device}, got {r.dtype} "
                             f"{tuple(r.shape)} on {r.device}")
        r = r.contiguous()
        n = r.shape[0]
        if int(cap) != cap or not 0 <= int(cap) <= 10:
            raise ValueError(f"lookup: cap must be in 0..10, got {cap!r}")
        if cube is not None:
            cube = torch.as_tensor(cube)
            if cube.shape != (n,) or cube.dtype != torch.uint8 or cube.device != self.device:
                raise ValueError(f"lookup: cube must be uint8[{n}] on {self.device}")
            cube = cube.contiguous()
        if out is None:
            out = (torch.empty(n, dtype=torch.uint8, device=self.device),
                   torch.full((n, 4), float("nan"), dtype=torch.float32, device=self.device),
                   torch.empty(n, dtype=torch.uint8, device=self.device))
        in_db, values, flags = out
        check(self._lib.bgx_bearoff_cube_lookup(self._h, _ptr(r), _ptr(cube), n, int(cap), _ptr(in_db), _ptr(values),
                                                _ptr(flags), _stream(self.device)), "bgx_bearoff_cube_lookup")
        return in_db, values, flags


# ------------------------------------------------------------- host references --
CUBE_CHILD = (0, 2, 1)              # the cube state the next roller sees: cen -> cen, own -> opp, opp -> own


def cube_table_reference(succ, n: int, dtype=np.float32):
    """(equity[3, n, n], nd[2, n, n]) of the cubeful table on the host, from successor sets given
    as for table_reference, by the recurrence of include/bgx.h with every product and sum
    rounded to `dtype` once, the rolls in order from 0: np.float32 gives the device table's bits,
    np.float64 a reference for its rounding error."""
    f = dtype
    E, ND = np.zeros((3, n, n), f), np.zeros((2, n, n), f)
    for x in (E, ND):
        x[:, :, 0] = f(-1)
        x[:, 0, 1:] = f(1)
    p = ROLL_P.astype(f) if f is np.float32 else np.array([1 / 36 if a == b else 2 / 36 for a, b in ROLLS21], f)
    flat = [[np.asarray(s, np.int64) for s in succ[a]] for a in range(n)]
    depth = np.zeros(n, np.int64)                           # table_reference's level function
    for a in range(1, n):
        depth[a] = 1 + max(depth[int(x)] for s in flat[a] for x in s)
    by_depth = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]
    for t in range(2, 2 * len(by_depth) - 1):
        for a in range(1, n):
            db = t - int(depth[a])
            if not 1 <= db < len(by_depth):
                continue
            bs = by_depth[db]                               # every b of this level at once
            acc = np.zeros((3, len(bs)), f)
            for r in range(21):
                s = flat[a][r]
                for st in range(3):
                    v = np.where(s == 0, f(1), -E[CUBE_CHILD[st]][np.ix_(bs, s)]).astype(f).max(axis=1)
                    acc[st] = (acc[st] + (p[r] * v).astype(f)).astype(f)
            cash = np.minimum((f(2) * acc[2]).astype(f), f(1))
            ND[0, a, bs], ND[1, a, bs] = acc[0], acc[1]
            E[0, a, bs], E[1, a, bs], E[2, a, bs] = np.maximum(acc[0], cash), np.maximum(acc[1], cash), acc[2]
    return E, ND


def cube_values_reference(state, nd_s, e_opp, w):
    """Part 1 of csrc/bg_bearoff_cube.h on arrays: (values f32[..., 4], flags uint8[...]) from
    the cube state (0 cen, 1 own, 2 opp, 3 dead), nd_s = ND_state[a][b] (read for cen and own
    only), e_opp = E_opp[a][b] and w = W[a][b]."""
    f = np.float32
    state, nd_s, e_opp, w = np.broadcast_arrays(np.asarray(state), np.asarray(nd_s, f), np.asarray(e_opp, f),
                                                np.asarray(w, f))
    with np.errstate(invalid="ignore", over="ignore"):
        dt = (f(2) * e_opp).astype(f)
        cl = ((f(2) * w).astype(f) - f(1)).astype(f)
        access = state <= 1
        nd = np.where(access, nd_s, np.where(state == 2, e_opp, cl)).astype(f)
        cash = np.where(dt < f(1), dt, f(1)).astype(f)
        doubles = access & (cash > nd)
        takes = dt <= f(1)
    values = np.stack([nd, dt, np.where(doubles, cash, nd).astype(f), cl], axis=-1)
    flags = (access * 1 + doubles * 2 + takes * 4 + (state == 3) * 8).astype(np.uint8)
    return values, flags


def cube_state_reference(cube, cap: int, mover):
    """(state, k) of cube bytes for the record's mover (0 / 1): k as min(k, cap), owner 3 as 0;
    k >= cap is dead (3), owner 0 cen (0), owner mover + 1 own (1), otherwise opp (2)."""
    c, m = np.asarray(cube).astype(np.int64), np.asarray(mover).astype(np.int64) & 1
    k, o = np.minimum(c & 15, int(cap)), (c >> 4) & 3
    o = np.where(o == 3, 0, o)
    return np.where(k >= int(cap), 3, np.where(o == 0, 0, np.where(o == m + 1, 1, 2))), k


def cube_fixed_reference(v, start_mover_on_roll, k):
    """boc_fixed of csrc/bg_bearoff_cube.h on arrays: Yq = clamp(rint(fp32(+-v 2^20)), +-2^20) 2^k,
    0 for a NaN (round half even)."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.where(start_mover_on_roll, np.asarray(v, f), -np.asarray(v, f)).astype(f) * f(1 << 20)).astype(f)
    x = np.where(np.isnan(x), f(0), np.clip(x, -float(1 << 20), float(1 << 20)))
    return np.rint(x).astype(np.int64) * (np.int64(1) << np.asarray(k).astype(np.int64))


def cube_lookup_reference(records, configs, equity, nd, table, max_checkers: int, cube=None, cap: int = 6):
    """bgx_bearoff_cube_lookup on the host: (in_db bool[n], values f32[n, 4], NaN where not in the
    table, flags uint8[n], 0 there) for uint8 [n, 64] records, with `configs`, `equity`, `nd` as
    CubefulBearoffDB publishes them and `table` = the cubeless W."""
    r = np.asarray(records).astype(np.int64)
    equity, nd = np.asarray(equity, np.float32), np.asarray(nd, np.float32)
    in_db, _ = lookup_reference(records, configs, table, max_checkers)
    index = {tuple(int(v) for v in c): i for i, c in enumerate(np.asarray(configs))}
    c0, c1 = r[:, 23:17:-1], r[:, 24:30]
    n = r.shape[0]
    m = r[:, R_CUR] & 1
    state, _ = cube_state_reference(np.zeros(n, np.uint8) if cube is None else cube, cap, m)
    values, flags = np.full((n, 4), np.nan, np.float32), np.zeros(n, np.uint8)
    table = np.asarray(table, np.float32)
    on = np.nonzero(in_db)[0]
    if on.size:
        idx = np.array([(index[tuple(c0[i])], index[tuple(c1[i])]) for i in on], np.int64)
        a, b = idx[np.arange(on.size), m[on]], idx[np.arange(on.size), 1 - m[on]]
        st = state[on]
        values[on], flags[on] = cube_values_reference(st, np.where(st <= 1, nd[np.minimum(st, 1), a, b], np.float32(0)),
                                                      equity[2, a, b], table[a, b])
    return in_db, values, flags


def dist_reference(succ, n: int):
    """(dist f32[n, 32], surv f32[n, 32], mean f32[n], choice int32[n, 21]) of the one-sided
    table on the host, from successor sets given as index lists as for table_reference (index
    0 = the empty configuration, every play leads to a smaller index; duplicates do not
    matter), by the recurrence of include/bgx.h in numpy float32, every product, difference and
    sum rounded once: the device table's bits."""
    f = np.float32
    dist, surv = np.zeros((n, ROW), f), np.zeros((n, ROW), f)
    mean, choice = np.zeros(n, f), np.zeros((n, 21), np.int32)
    dist[0, 0] = surv[0, 0] = f(1)
    for a in range(1, n):
        for r in range(21):
            choice[a, r] = min((mean[int(x)], int(x)) for x in succ[a][r])[1]
        dist[a], surv[a], mean[a] = row_reference(dist[choice[a]])
    return dist, surv, mean, choice


def row_reference(rows):
    """One configuration's (dist f32[32], surv f32[32], mean f32) from the f32[21, 32] rows of
    its 21 chosen successors: the recurrence's step for one a."""
    f = np.float32
    acc = np.zeros(ROW - 1, f)
    for r in range(21):
        acc = (acc + (ROLL_P[r] * np.asarray(rows[r], f)[:-1]).astype(f)).astype(f)
    d = np.concatenate([np.zeros(1, f), acc])
    s = np.ones(ROW, f)
    m = f(0)
    for t in range(1, ROW):
        m = f(m + f(f(t) * d[t]))
        if t + 1 < ROW:
            s[t + 1] = f(s[t] - d[t])
    return d, s, m


def win1_reference(dist_x, surv_y) -> np.ndarray:
    """win1(x on roll, y) = sum over t = 1..31, in that order from 0, of D[x][t] S[y][t] in numpy
    float32 for rows dist_x f32[..., 32] of x and surv_y f32[..., 32] of y (broadcast together)."""
    f = np.float32
    dx, sy = np.asarray(dist_x, f), np.asarray(surv_y, f)
    acc = np.zeros(np.broadcast(dx[..., 0], sy[..., 0]).shape, f)
    for t in range(1, ROW):
        acc = (acc + (dx[..., t] * sy[..., t]).astype(f)).astype(f)
    return acc


def lookup1_reference(records, configs, dist, surv, max_checkers: int):
    """bgx_bearoff1_lookup on the host: (in_db uint8[n] in {0, 1, 2}, win f32[n], NaN where not
    in the table) for uint8 [n, 64] records, with `configs`, `dist` and `surv` as
    OneSidedBearoffDB publishes them."""
    r = np.asarray(records).astype(np.int64)
    configs, K = np.asarray(configs), int(max_checkers)
    dist, surv = np.asarray(dist, np.float32), np.asarray(surv, np.float32)
    index = {tuple(int(v) for v in c): i for i, c in enumerate(configs)}
    c0, c1 = r[:, 23:17:-1], r[:, 24:30]                      # distances 1..6 of PLAYER1 / PLAYER2
    h0, h1 = c0.sum(1), c1.sum(1)
    inside = ((r[:, R_OVER] == 0) & (r[:, 48] == 0) & (r[:, 49] == 0) & (r[:, 0:18].sum(1) == 0) &
              (r[:, 30:48].sum(1) == 0) & (h0 >= 1) & (h0 <= K) & (h1 >= 1) & (h1 <= K) &
              (h0 + r[:, 50] == 15) & (h1 + r[:, 51] == 15))
    in_db = np.where(inside, np.where((h0 < 15) & (h1 < 15), 1, 2), 0).astype(np.uint8)
    win = np.full(r.shape[0], np.nan, np.float32)
    for i in np.nonzero(inside)[0]:
        idx = (index[tuple(c0[i])], index[tuple(c1[i])])
        m = int(r[i, R_CUR]) & 1
        win[i] = win1_reference(dist[idx[m]], surv[idx[1 - m]])
    return in_db, win


def lookup_reference(records, configs, table, max_checkers: int):
    """bgx_bearoff_lookup on the host: (in_db bool[n], win f32[n], NaN where not in the table)
    for uint8 [n, 64] records, with `configs` int8[n_cfg, 6] and `table` f32[n_cfg, n_cfg] as
    BearoffDB publishes them."""
    r = np.asarray(records).astype(np.int64)
    configs, table, K = np.asarray(configs), np.asarray(table, np.float32), int(max_checkers)
    index = {tuple(int(v) for v in c): i for i, c in enumerate(configs)}
    c0, c1 = r[:, 23:17:-1], r[:, 24:30]                      # distances 1..6 of PLAYER1 / PLAYER2
    h0, h1 = c0.sum(1), c1.sum(1)
    in_db = ((r[:, R_OVER] == 0) & (r[:, 48] == 0) & (r[:, 49] == 0) & (r[:, 0:18].sum(1) == 0) &
             (r[:, 30:48].sum(1) == 0) & (h0 >= 1) & (h0 <= K) & (h1 >= 1) & (h1 <= K) &
             (h0 + r[:, 50] == 15) & (h1 + r[:, 51] == 15))
    win = np.full(r.shape[0], np.nan, np.float32)
    for i in np.nonzero(in_db)[0]:
        idx = (index[tuple(c0[i])], index[tuple(c1[i])])
        m = int(r[i, R_CUR]) & 1
        win[i] = table[idx[m], idx[1 - m]]
    return in_db, win


def table_reference(succ, n: int, dtype=np.float32) -> np.ndarray:
    """W[n, n] on the host from successor sets given as index lists, succ[a][r] for
    configuration a and roll r (index 0 = the empty configuration; every play leads to a
    smaller index, as any order by pip count ensures), by the recurrence of include/bgx.h with
    every subtraction, product and sum rounded to `dtype` once, the rolls in order from 0:
    np.float32 gives the device table's bits, np.float64 a reference for its rounding error."""
    f = dtype
    W = np.zeros((n, n), f)
    W[0, 1:] = f(1)
    p = ROLL_P.astype(f) if f is np.float32 else np.array([1 / 36 if a == b else 2 / 36 for a, b in ROLLS21], f)
    flat = [[np.asarray(s, np.int64) for s in succ[a]] for a in range(n)]
    # a level function that falls along every play, like the pip count: the longest chain of
    # plays to the empty configuration.  W[a][b] needs W[b][a'] of a smaller level sum only.
    depth = np.zeros(n, np.int64)
    for a in range(1, n):
        depth[a] = 1 + max(depth[int(x)] for s in flat[a] for x in s)
    by_depth = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]
    for t in range(2, 2 * len(by_depth) - 1):
        for a in range(1, n):
            db = t - int(depth[a])
            if not 1 <= db < len(by_depth):
                continue
            bs = by_depth[db]                               # every b of this level at once
            acc = np.zeros(len(bs), f)
            for r in range(21):
                s = flat[a][r]
                v = np.where(s == 0, f(1), f(1) - W[np.ix_(bs, s)]).astype(f).max(axis=1)
                acc = (acc + (p[r] * v).astype(f)).astype(f)
            W[a, bs] = acc
    return W
