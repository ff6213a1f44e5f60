"""The speed factor on the HIP device (csrc/timescale.hip, DESIGN.md "Speed factor"): the reference application's time-scaling
(``np.interp`` over ``np.linspace`` positions, speed clamped to [0.1, 5]; it moves the pitch with the tempo) and a pitch-preserving
mode, WSOLA (waveform-similarity overlap-add, Verhelst & Roelands 1993), which is also the one that can stream.

Host side only: the plan's integer arithmetic (output length, frames, nominal centres in float64, what a stream may decide from the
samples it has), the Hann window in float64, and the coverage check in front of every launch.  All arithmetic on samples happens in
the library (dia_timescale).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as hb

MIN_SPEED, MAX_SPEED = 0.1, 5.0      # the reference application's clamp
MODES = ("interp", "wsola")
MIN_WINDOW, MAX_WINDOW = 64, 4096    # DIA_TS_MIN_WINDOW / DIA_TS_MAX_WINDOW
MAX_ROWS = 64                        # DIA_TS_MAX_ROWS: rows of one launch
MAX_T = 1 << 24                      # DIA_TS_MAX_T: samples per row of one launch, in and out


def clamp_speed(speed: float) -> float:
    s = float(speed)
    if not math.isfinite(s):
        raise ValueError(f"time scale: speed = {speed} is not a finite number")
    return min(max(s, MIN_SPEED), MAX_SPEED)


@dataclass(frozen=True)
class TimescalePlan:
    """one (speed, mode, window, tolerance): `speed` is kept clamped.  Frame k of WSOLA is centred at output k * hop and nominally at
    input centre(k); it is searched over centre(k) + [-tolerance, tolerance]."""
    speed: float
    mode: str = "interp"
    window: int = 1024
    tolerance: int = 512

    def __post_init__(self):
        object.__setattr__(self, "speed", clamp_speed(self.speed))
        if self.mode not in MODES:
            raise ValueError(f"time scale: mode = {self.mode!r} is not one of {MODES}")
        W, D = int(self.window), int(self.tolerance)
        if W < MIN_WINDOW or W > MAX_WINDOW or W & (W - 1):
            raise ValueError(f"time scale: window = {self.window} is not a power of two in [{MIN_WINDOW}, {MAX_WINDOW}]")
        if D < 0 or D > W:
            raise ValueError(f"time scale: tolerance = {self.tolerance} outside [0, window = {W}]")
        object.__setattr__(self, "window", W)
        object.__setattr__(self, "tolerance", D)

    @property
    def hop(self) -> int:
        return self.window // 2

    @property
    def identity(self) -> bool:
        return self.speed == 1.0

    def out_len(self, N: int) -> int:
        """outputs of a signal of N samples: int(N / speed) in float64, as the reference"""
        return int(int(N) / self.speed)

    def passes(self, N: int) -> bool:
        """the signal comes back unchanged, with no launch"""
        M = self.out_len(N)
        return self.identity or M <= 0 or (self.mode == "interp" and M == int(N))

    def frames(self, M: int) -> int:
        """frames 0 .. F - 1 of M outputs: every output has exactly two"""
        return -(-int(M) // self.hop) + 1

    def centre(self, k: int) -> int:
        """c_k = floor(k * hop * speed + 0.5) in float64; depends on k alone"""
        return int(math.floor(float(int(k) * self.hop) * self.speed + 0.5))

    def centres(self, k0: int, k1: int) -> np.ndarray:
        """centre(k) of k in [k0, k1), int64"""
        k = np.arange(int(k0), int(k1), dtype=np.int64) * self.hop
        return np.floor(k.astype(np.float64) * self.speed + 0.5).astype(np.int64)

    def need(self, k: int) -> int:
        """input samples [0, need) that deciding frame k may read: its candidates reach centre(k) + tolerance + hop, its template,
        the continuation of frame k - 1's segment, centre(k - 1) + tolerance + window (the larger one when speed < 1)"""
        if k <= 0:
            return self.hop
        return max(self.centre(k) + self.tolerance + self.hop, self.centre(k - 1) + self.tolerance + self.window)

    def ready_frames(self, got: int) -> int:
        """how many frames [0, K) of an open signal can be decided from its first `got` samples"""
        lo, hi = 0, int(int(got) / (self.hop * self.speed)) + 2                # need(hi) > got
        while lo < hi:
            mid = (lo + hi) // 2
            if self.need(mid) <= got:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def span(self, k0: int, k1: int) -> Tuple[int, int]:
        """[lo, hi): every input index that searching frames [k0, k1) and overlap-adding frames k0 - 1 .. k1 - 1 can read, whatever
        the offsets turn out to be (lo may be negative)"""
        first = max(int(k0) - 1, 0)
        lo = self.centre(first) - self.tolerance - self.hop
        hi = max(self.need(k) for k in (max(int(k1) - 1, 0), first))
        return lo, hi


def hann(window: int) -> np.ndarray:
    """the periodic Hann window in float64: w[n] + w[n + window / 2] = 1"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(window), dtype=np.float64) / int(window))


def check_coverage(plan: TimescalePlan, in_start: int, in_count: int, k0: int, k1: int, out_start: int, out_count: int,
                   total: Optional[int]) -> None:
    """WSOLA: the outputs lie in the range of the frames, and every input sample inside [0, total) that the launch can read lies in
    the window [in_start, in_start + in_count): the kernel treats everything else as zero, so a sample not supplied would
    silently read as 0"""
    if k1 < k0 or k0 < 0:
        raise ValueError(f"time scale: frames [{k0}, {k1}) are not a range")
    if out_count > 0 and (out_start < (k0 - 1) * plan.hop or out_start + out_count > (k1 - 1) * plan.hop):
        raise ValueError(f"time scale: outputs [{out_start}, {out_start + out_count}) lie outside the range of frames [{k0 - 1}, {k1})")
    if k1 == k0:
        return
    lo, hi = plan.span(k0, k1)
    lo = max(lo, 0)
    if total is not None:
        hi = min(hi, int(total))
    if lo < hi and (lo < in_start or hi > in_start + in_count):
        raise ValueError(f"time scale: frames [{k0}, {k1}) read input samples [{lo}, {hi}), the window holds [{in_start}, {in_start + in_count})")


# run(window, in_start, k0, k1, delta_prev, out_start, out_count, total) -> (delta int [k1 - k0], float32 [out_count])
RunFn = Callable[[np.ndarray, int, int, int, int, int, int, Optional[int]], Tuple[np.ndarray, np.ndarray]]


class TimescaleStream:
    """Streaming WSOLA of one signal: push() takes consecutive chunks of input samples and returns every output sample both of whose
    frames are decided; the state is the input tail later frames still read, the offset of the last decided frame and the count
    handed out.  Every correlation and every output is the same chain on the same samples as in a whole-signal run, so the chunks
    joined equal it bit for bit.  (The interpolating mode cannot stream: its positions depend on the total length.)"""

    def __init__(self, plan: TimescalePlan, run: RunFn):
        if plan.mode != "wsola":
            raise ValueError("time scale: mode 'interp' cannot stream: every position j * (N - 1) / (M - 1) depends on the signal's "
                             "total length N, which a stream learns last; use mode='wsola'")
        self.plan, self.run = plan, run
        self.buf = np.zeros(0, dtype=np.float32)                # samples [base, got)
        self.base = 0
        self.got = 0
        self.decided = 0                                        # frames [0, decided) have their offsets
        self.delta_last = 0                                     # offset of frame decided - 1
        self.emitted = 0                                        # outputs handed out so far: the start offset of the next chunk
        self.final = False

    def push(self, chunk, final: bool = False) -> np.ndarray:
        if self.final:
            raise RuntimeError("TimescaleStream: push() after the final chunk")
        p = self.plan
        c = np.asarray(chunk, dtype=np.float32).reshape(-1)
        self.buf = np.concatenate([self.buf, c])
        self.got += c.shape[0]
        self.final = bool(final)
        if final:
            M = p.out_len(self.got)
            if M <= 0:                                          # as time_scale(): the input comes back (nothing was handed out before)
                return self.buf.copy()
            k_end, out_end = p.frames(M), M
        else:
            k_end = max(self.decided, p.ready_frames(self.got))
            out_end = max(self.emitted, (k_end - 1) * p.hop)
        parts = []
        # a launch takes at most MAX_T samples per row, in and out
        step = max(2, (MAX_T - 2 * p.window - 2 * p.tolerance - 2) // (int(p.hop * max(p.speed, 1.0)) + 1) - 2)
        while self.decided < k_end:
            k0, k1 = self.decided, min(k_end, self.decided + step)
            o1 = max(self.emitted, min(out_end, (k1 - 1) * p.hop))
            lo, hi = p.span(k0, k1)
            lo = min(max(self.base, lo), self.got)
            hi = min(self.got, max(lo, hi))
            delta, y = self.run(self.buf[lo - self.base:hi - self.base], lo, k0, k1, self.delta_last, self.emitted, o1 - self.emitted,
                                self.got if final else None)
            parts.append(y)
            self.delta_last = int(delta[-1])
            self.decided, self.emitted = k1, o1
        keep = min(self.got, max(self.base, p.span(self.decided, self.decided)[0]))      # earlier samples are never read again
        if keep > self.base:
            self.buf = self.buf[keep - self.base:].copy()
            self.base = keep
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


class _Identity:
    """the stream of speed 1: chunks pass through"""

    def __init__(self):
        self.emitted, self.final = 0, False

    def push(self, chunk, final: bool = False) -> np.ndarray:
        if self.final:
            raise RuntimeError("TimescaleStream: push() after the final chunk")
        self.final = bool(final)
        c = np.asarray(chunk, dtype=np.float32).reshape(-1)
        self.emitted += c.shape[0]
        return c


# ---------------------------------------------------------------------------------------------- the device side
def _fn():
    return hb.lib().dia_timescale


def _i64(v: Sequence[int]):
    return (C.c_int64 * len(v))(*[int(u) for u in v])


def _i32(v: Sequence[int]):
    return (C.c_int32 * len(v))(*[int(u) for u in v])


class DeviceTimescale:
    """dia_timescale on one HIP device: the window is uploaded once per size; every call goes host to device to host.  There is no
    CPU fallback."""

    def __init__(self, device=None):
        import torch

        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        _fn()
        self._wins: dict = {}

    def _win(self, window: int):
        import torch

        if window not in self._wins:
            self._wins[window] = torch.from_numpy(hann(window).astype(np.float32)).to(self.device)
        return self._wins[window]

    def _call(self, a: "hb.TimescaleArgs") -> None:
        import torch

        with torch.cuda.device(self.device):
            hb.check(_fn()(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_timescale")

    def launch_interp(self, x, y, in_start, in_count, out_start, out_count, total, out_total) -> None:
        """one DIA_TS_INTERP launch on device tensors x fp32 [B, ldx] -> y fp32 [B, ldy], B <= MAX_ROWS: row b holds input samples
        [in_start[b], + in_count[b]) of a signal of total[b] samples and receives outputs [out_start[b], + out_count[b]) of its
        out_total[b]"""
        B = x.shape[0]
        self._call(hb.TimescaleArgs(x=hb.ptr(x), y=hb.ptr(y), mode=hb.TS_INTERP, B=B, ldx=x.shape[1], ldy=y.shape[1],
                                    in_start=_i64(in_start), out_start=_i64(out_start), total=_i64(total), out_total=_i64(out_total),
                                    in_count=_i32(in_count), out_count=_i32(out_count)))

    def launch_wsola(self, plan: TimescalePlan, x, y, centre, delta, in_start, in_count, k0, k1, delta_prev, out_start, out_count,
                     total) -> None:
        """one DIA_TS_WSOLA launch (search, then overlap-add) on device tensors x fp32 [B, ldx] -> y fp32 [B, ldy] and delta int32
        [B, ldk], with centre int32 [B, ldk + 1] = plan.centre(k) - in_start[b] of frames k0[b] - 1 .. k1[b]; total[b] None: open"""
        B = x.shape[0]
        for b in range(B):
            check_coverage(plan, int(in_start[b]), int(in_count[b]), int(k0[b]), int(k1[b]), int(out_start[b]), int(out_count[b]),
                           None if total[b] is None else int(total[b]))
        self._call(hb.TimescaleArgs(x=hb.ptr(x), y=hb.ptr(y), win=hb.ptr(self._win(plan.window)), centre=hb.ptr(centre), delta=hb.ptr(delta),
                                    mode=hb.TS_WSOLA, B=B, ldx=x.shape[1], ldy=y.shape[1], ldk=delta.shape[1],
                                    window=plan.window, tolerance=plan.tolerance,
                                    in_start=_i64(in_start), out_start=_i64(out_start),
                                    total=_i64([hb.TS_OPEN if v is None else v for v in total]), k0=_i64(k0), k1=_i64(k1),
                                    delta_prev=_i32(delta_prev), in_count=_i32(in_count), out_count=_i32(out_count)))

    def run_rows(self, plan: TimescalePlan, buf: np.ndarray, in_start, in_count, k0, k1, delta_prev, out_start, out_count,
                 total) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """host rows buf [B, ld] (whatever lies beyond in_count[b] is never read) through launches of at most MAX_ROWS rows ->
        (float32 [out_count[b]], int32 delta [k1[b] - k0[b]]) per row.  interp: total[b] is the signal's length, its outputs number
        plan.out_len(total[b]), and k0 / k1 / delta_prev are not read."""
        import torch

        buf = np.ascontiguousarray(buf, dtype=np.float32)
        ys: List[np.ndarray] = []
        ds: List[np.ndarray] = []
        for g0 in range(0, buf.shape[0], MAX_ROWS):
            sl = slice(g0, min(buf.shape[0], g0 + MAX_ROWS))
            x = torch.from_numpy(buf[sl]).to(self.device)
            B = x.shape[0]
            y = torch.empty(B, max(1, max(out_count[sl])), dtype=torch.float32, device=self.device)
            if plan.mode == "interp":
                self.launch_interp(x, y, in_start[sl], in_count[sl], out_start[sl], out_count[sl], total[sl],
                                   [plan.out_len(v) for v in total[sl]])
                nk = [0] * B
                dh = np.zeros((B, 0), dtype=np.int32)
            else:
                nk = [int(b) - int(a) for a, b in zip(k0[sl], k1[sl])]
                ldk = max(1, max(nk))
                ch = np.zeros((B, ldk + 1), dtype=np.int32)
                for r in range(B):                              # entry i: frame k0 - 1 + i; frame -1 does not exist
                    a, lead = int(k0[sl][r]), int(k0[sl][r]) == 0
                    ch[r, lead:nk[r] + 1] = plan.centres(a - 1 + lead, a + nk[r]) - int(in_start[sl][r])
                centre = torch.from_numpy(ch).to(self.device)
                delta = torch.zeros(B, ldk, dtype=torch.int32, device=self.device)
                self.launch_wsola(plan, x, y, centre, delta, in_start[sl], in_count[sl], k0[sl], k1[sl], delta_prev[sl], out_start[sl],
                                  out_count[sl], total[sl])
                dh = delta.cpu().numpy()
            yh = y.cpu().numpy()
            ys.extend(yh[r, :c].copy() for r, c in enumerate(out_count[sl]))
            ds.extend(dh[r, :n].copy() for r, n in enumerate(nk))
        return ys, ds

    def time_scale(self, waves, speed: float, mode: str = "interp", window: int = 1024, tolerance: int = 512, return_delta: bool = False):
        """one mono float array [N], or a list of them with their own lengths (one launch per MAX_ROWS rows), stretched to
        float32 [int(N / speed)] each: speed < 1 is slower.  mode "interp" is the reference application's method (the pitch moves
        with the tempo), "wsola" keeps the pitch.  speed 1 (after the clamp to [0.1, 5]), no output, or interp with as many outputs
        as inputs return the input unchanged with no launch.  return_delta: also the rows' WSOLA offsets (int32 [frames])."""
        plan = TimescalePlan(speed, mode, window, tolerance)
        single = not isinstance(waves, (list, tuple))
        rows = []
        for w in ([waves] if single else waves):
            a = np.asarray(w.detach().cpu() if hasattr(w, "detach") else w)
            if a.ndim == 2 and a.shape[0] == 1:
                a = a[0]
            if a.ndim != 1 or a.dtype.kind != "f":
                raise ValueError(f"time scale: a waveform of shape {tuple(a.shape)} and dtype {a.dtype}, expected mono float samples [N]")
            rows.append((w, a))
        out: list = [w for w, _ in rows]
        deltas: list = [np.zeros(0, dtype=np.int32) for _ in rows]
        at = [i for i, (_, a) in enumerate(rows) if not plan.passes(a.shape[0])]
        if at:
            lens = [rows[i][1].shape[0] for i in at]
            M = [plan.out_len(n) for n in lens]
            if max(lens) > MAX_T or max(M) > MAX_T:
                raise ValueError(f"time scale: more than {MAX_T} samples per row; use stream()")
            buf = np.empty((len(at), max(lens)), dtype=np.float32)            # what lies behind a row is never read
            for b, i in enumerate(at):
                buf[b, :lens[b]] = rows[i][1]
            zero = [0] * len(at)
            ys, ds = self.run_rows(plan, buf, zero, lens, zero, [plan.frames(m) for m in M], zero, zero, M, lens)
            for b, i in enumerate(at):
                out[i], deltas[i] = ys[b], ds[b]
        if return_delta:
            return (out[0], deltas[0]) if single else (out, deltas)
        return out[0] if single else out

    def stream(self, speed: float, window: int = 1024, tolerance: int = 512, mode: str = "wsola"):
        """a streaming state for one signal on this device (WSOLA only: TimescaleStream says why)"""
        plan = TimescalePlan(speed, mode, window, tolerance)
        if plan.mode != "wsola":
            TimescaleStream(plan, None)                         # raises
        if plan.identity:
            return _Identity()

        def run(win: np.ndarray, in_start: int, k0: int, k1: int, delta_prev: int, out_start: int, out_count: int, total: Optional[int]):
            buf = win[None] if win.shape[0] else np.zeros((1, 1), dtype=np.float32)
            ys, ds = self.run_rows(plan, buf, [in_start], [win.shape[0]], [k0], [k1], [delta_prev], [out_start], [out_count], [total])
            return ds[0], ys[0]

        return TimescaleStream(plan, run)
