"""1-ply greedy and 2-ply expectimax move selection over engine lanes
(the reference's intended moves/expect_minmax.py, which is
commented out there).  V = value_head(relu(fc1 x)) of a
BackgammonPolicyNetwork (policy_network.py:54-56), H <= 128 (C2/C4 use H = 40;
the reference trains H = 128, agent/config.py:8).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check
from .engine import Engine, _ptr, _stream


class ValueHead:
    """Packed (fc1, value_head) of a policy network for the search kernels."""

    def __init__(self, net):
        L = _lib.load()
        self.hidden = net.fc1.out_features
        n = L.bgx_value_packed_size(self.hidden)
        if n < 0:
            raise ValueError(f"value search supports hidden <= 128 (got {self.hidden})")
        dev = net.fc1.weight.device
        ps = [t.detach().float().contiguous() for t in (net.fc1.weight, net.fc1.bias, net.value_head.weight,
                                                         net.value_head.bias)]
        self.packed = torch.empty(n, dtype=torch.float32, device=dev)
        check(L.bgx_value_pack(*[_ptr(t) for t in ps], self.hidden, _ptr(self.packed), _stream(dev)),
              "bgx_value_pack")
        self.bias = float(net.value_head.bias.detach().float().cpu()[0])


def _check_sel(eng: Engine, sel):
    if sel is None:
        return
    if (not isinstance(sel, torch.Tensor) or sel.dtype != torch.uint8 or sel.device != eng.device
            or not sel.is_contiguous() or sel.numel() != eng.batch):
        raise ValueError("sel must be a contiguous uint8[B] tensor on the engine's device")


def _outputs(eng: Engine, out, what: str):
    """(best int32[B], best value f32[B], values f32[B, max_moves] or None) given by the
    caller: a lane-selected call writes the selected lanes' entries only."""
    best, bestv, vals = out
    for t, dt, n in ((best, torch.int32, eng.batch), (bestv, torch.float32, eng.batch),
                     (vals, torch.float32, eng.batch * eng.max_moves)):
        if t is not None and (t.dtype != dt or t.device != eng.device or not t.is_contiguous() or t.numel() != n):
            raise ValueError(f"{what}: out must be contiguous (int32[B], float32[B], float32[B, max_moves] or None) "
                             "on the engine's device")
    if best is None or bestv is None:
        raise ValueError(f"{what}: out needs the best and best-value tensors")
    return best, bestv, vals


def one_ply(eng: Engine, vh: ValueHead, want_values: bool = False, sel: torch.Tensor | None = None, out=None):
    """First argmax over each lane's afterstates of V(afterstate, mover one-hot).
    `sel` (uint8[B] on the device): only lanes with sel != 0 are searched and written
    (bgx_one_ply_sel); the other lanes' entries keep what they held -- pass `out` =
    (best, bestv, values or None) to choose that, else they are uninitialised
    (values: NaN)."""
    L = _lib.load()
    B, dev = eng.batch, eng.device
    _check_sel(eng, sel)
    if out is not None:
        best, bestv, vals = _outputs(eng, out, "one_ply")
        want_values = vals is not None
    else:
        best = torch.empty(B, dtype=torch.int32, device=dev)
        bestv = torch.empty(B, dtype=torch.float32, device=dev)
        vals = torch.full((B, eng.max_moves), float("nan"), dtype=torch.float32, device=dev) if want_values else None
    check(L.bgx_one_ply_sel(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(best), _ptr(bestv),
                            _ptr(vals), _stream(dev)), "bgx_one_ply_sel")
    return (best, bestv, vals) if want_values else (best, bestv)


def _ord_f32(v: torch.Tensor) -> torch.Tensor:
    """The order-preserving integer encoding of fp32 bits (csrc/bg_search.hip ord_f32)."""
    b = v.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(b >= 0, b, b ^ 0x7FFFFFFF)


def move_filter_reference(v1, n, top_k: int, margin: float) -> torch.Tensor:
    """The move filter's rule in plain torch (any device; the specification of the k_filter
    kernel behind bgx_two_ply_topk): the bool kept mask [B, max_moves] of 1-ply values
    v1 f32[B, max_moves] with n[B] legal moves per lane.  On the order-preserving integer
    encoding of the float bits,
        rank(a) = #{b : V1(b) > V1(a)} + #{b < a : V1(b) == V1(a)}
        keep(a) = rank(a) < top_k and (rank(a) == 0 or V1(a) >= fp32(V1best - margin));
    margin = inf: no threshold."""
    v1 = torch.as_tensor(v1, dtype=torch.float32)
    if v1.dim() != 2:
        raise ValueError("move_filter_reference: v1 must be [B, max_moves]")
    top_k, margin = int(top_k), float(margin)
    if top_k < 1 or not margin >= 0.0:
        raise ValueError(f"move_filter_reference: top_k {top_k} must be >= 1 and margin {margin} >= 0")
    B, M = v1.shape
    n = torch.as_tensor(n, device=v1.device).to(torch.int64).reshape(B)
    idx = torch.arange(M, device=v1.device)
    valid = idx[None, :] < n[:, None]
    key = _ord_f32(v1)
    # rank = position in the stable order by falling value (equal values: rising index);
    # entries a >= n sort behind every legal move
    order = torch.sort(torch.where(valid, -key, torch.full_like(key, 1 << 40)), dim=1, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(1, order, idx[None, :].expand(B, M).contiguous())
    keep = valid & (rank < top_k)
    if margin != float("inf") and M > 0:
        vbest = torch.gather(v1, 1, order[:, :1])                       # rank 0 (unused where n = 0)
        thr = _ord_f32(vbest - torch.tensor(margin, dtype=torch.float32, device=v1.device))
        keep &= (rank == 0) | (key >= thr)
    return keep


def two_ply(eng: Engine, vh: ValueHead, want_q: bool = False, sel: torch.Tensor | None = None, out=None,
            top_k: int | None = None, margin: float | None = None, want_v1: bool = False):
    """2-ply expectimax for every lane: returns (best int32[B], best Q f32[B],
    Q f32[B, max_moves] or None, stats {leaves, jobs, afterstates}).  `sel`
    (uint8[B] on the device): only lanes with sel != 0 form rows, are searched, written and
    counted in the stats (bgx_two_ply_sel); `out` = (best, bestq, q or None) as in one_ply.

    `top_k` / `margin`: the 1-ply move filter (bgx_two_ply_topk; move_filter_reference is its
    rule): only the top_k best 1-ply moves within margin of the best are searched; best is
    the first argmax of Q over them, Q of a legal move that was not searched is -inf, and
    stats["afterstates"] counts the searched moves and the stats gain "candidates", all the
    legal ones (an unfiltered call searches every candidate and reports no such entry).
    margin None = inf, top_k None with a margin = max_moves.  want_v1 (the filtered entry
    point with either option or neither): a fifth result, the 1-ply values f32[B, max_moves]
    (NaN where nothing was written)."""
    L = _lib.load()
    B, dev = eng.batch, eng.device
    _check_sel(eng, sel)
    if out is not None:
        best, bestq, q = _outputs(eng, out, "two_ply")
    else:
        best = torch.empty(B, dtype=torch.int32, device=dev)
        bestq = torch.empty(B, dtype=torch.float32, device=dev)
        q = torch.full((B, eng.max_moves), float("nan"), dtype=torch.float32, device=dev) if want_q else None
    if top_k is None and margin is None and not want_v1:
        stats = (ctypes.c_uint64 * 3)()
        check(L.bgx_two_ply_sel(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(best), _ptr(bestq),
                                _ptr(q), ctypes.cast(stats, ctypes.c_void_p), _stream(dev)), "bgx_two_ply_sel")
        return best, bestq, q, {"leaves": int(stats[0]), "jobs": int(stats[1]), "afterstates": int(stats[2])}
    v1 = torch.full((B, eng.max_moves), float("nan"), dtype=torch.float32, device=dev) if want_v1 else None
    stats = (ctypes.c_uint64 * 4)()
    check(L.bgx_two_ply_topk(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel),
                             eng.max_moves if top_k is None else int(top_k),
                             float("inf") if margin is None else float(margin), _ptr(best), _ptr(bestq), _ptr(q),
                             _ptr(v1), ctypes.cast(stats, ctypes.c_void_p), _stream(dev)), "bgx_two_ply_topk")
    st = {"leaves": int(stats[0]), "jobs": int(stats[1]), "afterstates": int(stats[2]), "candidates": int(stats[3])}
    return (best, bestq, q, st, v1) if want_v1 else (best, bestq, q, st)


def roll_luck(eng: Engine, vh: ValueHead, sel: torch.Tensor | None = None, out=None):
    """The luck of every lane's roll (bgx_roll_luck; DESIGN.md §10 "Luck adjustment"): with
    v_r = the best 1-ply value of the lane's mover for roll r (V of the position itself when
    it cannot move), mean = sum_r p_r v_r over the 21 rolls and luck = v of the roll the lane
    holds - mean.  Returns (luck f32[B], mean f32[B], stats {leaves, jobs, rows}).  `sel`
    (uint8[B] on the device) as in one_ply: only lanes with sel != 0 are computed and
    written; `out` = (luck, mean or None) keeps the other entries as they were, else they are
    NaN.  Synchronises the stream, as two_ply does."""
    L = _lib.load()
    B, dev = eng.batch, eng.device
    _check_sel(eng, sel)
    if out is not None:
        luck, mean = out
        for t in (luck, mean):
            if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()
                                  or t.numel() != B):
                raise ValueError("roll_luck: out must be contiguous (float32[B], float32[B] or None) on the "
                                 "engine's device")
        if luck is None:
            raise ValueError("roll_luck: out needs the luck tensor")
    else:
        luck = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
        mean = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    stats = (ctypes.c_uint64 * 3)()
    check(L.bgx_roll_luck(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(luck), _ptr(mean),
                          ctypes.cast(stats, ctypes.c_void_p), _stream(dev)), "bgx_roll_luck")
    return luck, mean, {"leaves": int(stats[0]), "jobs": int(stats[1]), "rows": int(stats[2])}


def roll_values(eng: Engine, vh: ValueHead, sel: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """roll_luck's 21 values themselves (bgx_roll_values): values f32[B, 21],
    values[i, r] = v_r, the best 1-ply value of lane i's mover for roll r in the 21 rolls' order
    (V of the position itself when it cannot move).  Returns (values, stats {leaves, jobs,
    rows}).  `sel` as in roll_luck: only lanes with sel != 0 are computed and written; `out`
    (float32[B, 21]) keeps the other rows as they were, else they are NaN.  Synchronises the
    stream, as roll_luck does."""
    L = _lib.load()
    B, dev = eng.batch, eng.device
    _check_sel(eng, sel)
    if out is None:
        out = torch.full((B, 21), float("nan"), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev
          or not out.is_contiguous() or out.shape != (B, 21)):
        raise ValueError("roll_values: out must be a contiguous float32[B, 21] tensor on the engine's device")
    stats = (ctypes.c_uint64 * 3)()
    check(L.bgx_roll_values(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(out),
                            ctypes.cast(stats, ctypes.c_void_p), _stream(dev)), "bgx_roll_values")
    return out, {"leaves": int(stats[0]), "jobs": int(stats[1]), "rows": int(stats[2])}


def value_lanes(records, vh: ValueHead, sel: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """The static value V(enc(X, m)) of lane records under `vh` (bgx_value_lanes):
    the board and the mover (byte 52) of each record, the value head's own output for them --
    what PolicyNet.act returns as its value.  `records`: an Engine (its lane records, read in
    place) or a contiguous uint8[n, 64] tensor on the head's device.  `sel` (uint8[n] there):
    only records with sel != 0 are evaluated and written (a stretch of lanes without a
    selected one costs next to nothing); `out` (float32[n]) keeps the other entries as they
    were, else they are NaN.  Sync-free and graph-capturable."""
    L = _lib.load()
    if isinstance(records, Engine):
        n, dev, rp = records.batch, records.device, ctypes.c_void_p(records.lanes_ptr())
    else:
        if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 2
                or records.shape[1] != 64 or not records.is_contiguous() or not records.is_cuda):
            raise ValueError("value_lanes: records must be an Engine or a contiguous uint8[n, 64] tensor on the GPU")
        n, dev, rp = records.shape[0], records.device, _ptr(records)
    if sel is not None and (not isinstance(sel, torch.Tensor) or sel.dtype != torch.uint8 or sel.device != dev
                            or not sel.is_contiguous() or sel.numel() != n):
        raise ValueError("value_lanes: sel must be a contiguous uint8[n] tensor on the records' device")
    if out is None:
        out = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.numel() != n:
        raise ValueError("value_lanes: out must be a contiguous float32[n] tensor on the records' device")
    check(L.bgx_value_lanes(rp, n, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(out), _stream(dev)),
          "bgx_value_lanes")
    return out


def two_ply_timings(eng: Engine):
    """(enumeration ms, evaluation ms) of the last two_ply call's first round,
    timed with HIP events on the caller's stream."""
    L = _lib.load()
    ms = (ctypes.c_float * 2)()
    check(L.bgx_two_ply_timings(eng._h, ctypes.cast(ms, ctypes.c_void_p)), "bgx_two_ply_timings")
    return float(ms[0]), float(ms[1])
