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
from .engine import Engine, _ptr


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


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


def two_ply(eng: Engine, vh: ValueHead, want_q: bool = False, sel: torch.Tensor | None = None, out=None):
    """2-ply expectimax for every lane: returns (best int32[B], best Q f32[B],
    Q f32[B, max_moves] or None, stats {leaves, jobs, afterstates}).  `sel` (uint8[B] on
    the device): only lanes with sel != 0 form rows, are searched, written and counted in
    the stats (bgx_two_ply_sel); `out` = (best, bestq, q or None) as in one_ply."""
    L = _lib.load()
    B, dev = eng.batch, eng.device
    _check_sel(eng, sel)
    if out is not None:
        best, bestq, q = _outputs(eng, out, "two_ply")
    else:
        best = torch.empty(B, dtype=torch.int32, device=dev)
        bestq = torch.empty(B, dtype=torch.float32, device=dev)
        q = torch.full((B, eng.max_moves), float("nan"), dtype=torch.float32, device=dev) if want_q else None
    stats = (ctypes.c_uint64 * 3)()
    check(L.bgx_two_ply_sel(eng._h, _ptr(vh.packed), vh.hidden, vh.bias, _ptr(sel), _ptr(best), _ptr(bestq), _ptr(q),
                            ctypes.cast(stats, ctypes.c_void_p), _stream(dev)), "bgx_two_ply_sel")
    return best, bestq, q, {"leaves": int(stats[0]), "jobs": int(stats[1]), "afterstates": int(stats[2])}


def two_ply_timings(eng: Engine):
    """(enumeration ms, evaluation ms) of the last two_ply call's first round,
    timed with HIP events on the caller's stream."""
    L = _lib.load()
    ms = (ctypes.c_float * 2)()
    check(L.bgx_two_ply_timings(eng._h, ctypes.cast(ms, ctypes.c_void_p)), "bgx_two_ply_timings")
    return float(ms[0]), float(ms[1])
