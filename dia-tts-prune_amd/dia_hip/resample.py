"""Sample-rate conversion on the HIP device (csrc/resample.hip, DESIGN.md "Resampler"): any-rate voice prompts on the way in
(reference dia/model.py:558-559, ``torchaudio.functional.resample(audio, sr, 44100)``) and any delivery rate on the way out.

The filter is torchaudio's published default (``sinc_interp_hann``, lowpass_filter_width 6, rolloff 0.99), restated here from its
formula; torchaudio itself is not needed and the restatement is unpinned against it (checked on properties: tests/test_resample_cpu.py).

Host side only: the polyphase bank in float64 (resample_plan), the integer planning of windows and streams, and the coverage check
in front of every launch.  All arithmetic on samples happens in the library (dia_resample).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import binding as hb

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
MAX_BANK_BYTES = 64 << 20            # the compact fp32 bank of one rate pair, n * nt * 4 bytes: refused above
TILE_OUTPUTS = 1024                  # DIA_RESAMPLE_TILE: consecutive outputs of one workgroup
MAX_TILE_FLOATS = 16000              # DIA_RESAMPLE_MAX_TILE_FLOATS: a workgroup's staged input span (62.5 KiB of LDS): refused above
MAX_ROWS = 64                        # DIA_RESAMPLE_MAX_ROWS: rows of one launch
MAX_T = 1 << 24                      # DIA_RESAMPLE_MAX_T: samples per row of one launch, in and out


@dataclass(frozen=True)
class ResamplePlan:
    """the polyphase filter of one rate pair in compact form: phase p keeps taps [first[p], first[p] + nt) relative to q * o, the
    run of taps strictly inside the window (|t| < 6) padded with exact zeros to the longest run `nt`"""
    rate_in: int
    rate_out: int
    o: int                           # rate_in / gcd
    n: int                           # rate_out / gcd: phases
    width: int
    nt: int
    first: np.ndarray                # int32 [n], nondecreasing, first[n - 1] <= first[0] + o
    bank: np.ndarray                 # float64 [n][nt]
    bank32: np.ndarray               # float32 [n][nt]: `bank` rounded

    @property
    def K(self) -> int:
        """taps per phase of the full form"""
        return 2 * self.width + self.o

    def out_len(self, L: int) -> int:
        return -(-self.n * int(L) // self.o)

    def pos(self, m: int) -> int:
        """absolute index of the input sample under tap 0 of output m (may be negative)"""
        q, p = divmod(int(m), self.n)
        return q * self.o + int(self.first[p])

    def tile_floats(self) -> int:
        """upper bound of the input span one workgroup stages: pos() rises by at most ceil(o / n) per output"""
        return -(-(TILE_OUTPUTS - 1) * self.o // self.n) + 2 + self.nt


_plans: Dict[Tuple[int, int], ResamplePlan] = {}


def resample_plan(rate_in: int, rate_out: int) -> ResamplePlan:
    """the plan of a rate pair, cached.  Refused by both rates: a compact bank above MAX_BANK_BYTES, and a ratio o / n at which one
    workgroup's input tile exceeds MAX_TILE_FLOATS."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f"resample: sample rates {rate_in} Hz -> {rate_out} Hz must be positive")
    key = (rate_in, rate_out)
    if key in _plans:
        return _plans[key]
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    K = 2 * width + o
    reach = LOWPASS_FILTER_WIDTH * o / base                     # |k - width - p o / n| < reach inside the window
    if n * max(1, math.floor(2 * reach) - 1) * 4 > MAX_BANK_BYTES:
        raise ValueError(f"resample: {rate_in} Hz -> {rate_out} Hz needs a filter bank of {n} phases x about {math.floor(2 * reach)} taps, "
                         f"above the {MAX_BANK_BYTES >> 20} MiB limit; convert through an intermediate rate")
    # a window of taps per phase that contains every tap with |t| < 6; t is evaluated exactly as in the full [n][K] form
    W = math.floor(2 * reach) + 5
    p = np.arange(n, dtype=np.int64)
    k0 = np.floor(width + p * o / n - reach).astype(np.int64) - 1
    k = k0[:, None] + np.arange(W, dtype=np.int64)[None, :]
    t = (-p.astype(np.float64)[:, None] / n + (k - width).astype(np.float64) / o) * base
    inside = (np.abs(t) < LOWPASS_FILTER_WIDTH) & (k >= 0) & (k < K)
    if not inside.any(axis=1).all() or inside[:, 0].any() or inside[:, -1].any():
        raise AssertionError(f"resample: the tap window of {rate_in} Hz -> {rate_out} Hz does not bracket the filter")
    lead = inside.argmax(axis=1)
    run = inside.sum(axis=1)
    nt = int(run.max())
    tc = np.clip(t, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    f = np.sinc(tc) * np.cos(np.pi * tc / (2 * LOWPASS_FILTER_WIDTH)) ** 2 * (base / o)       # np.sinc(x) = sin(pi x) / (pi x)
    f = np.where(inside, f, 0.0)
    at = lead[:, None] + np.arange(nt, dtype=np.int64)[None, :]
    bank = np.take_along_axis(f, np.minimum(at, W - 1), axis=1) * (at < W)
    first = (k0 + lead - width).astype(np.int32)
    if n * nt * 4 > MAX_BANK_BYTES:
        raise ValueError(f"resample: {rate_in} Hz -> {rate_out} Hz needs a filter bank of {n} phases x {nt} taps, above the "
                         f"{MAX_BANK_BYTES >> 20} MiB limit; convert through an intermediate rate")
    if np.any(np.diff(first) < 0) or int(first[-1]) > int(first[0]) + o:
        raise AssertionError(f"resample: tap offsets of {rate_in} Hz -> {rate_out} Hz are not monotone")
    plan = ResamplePlan(rate_in, rate_out, o, n, width, nt, first, np.ascontiguousarray(bank), bank.astype(np.float32))
    if plan.tile_floats() > MAX_TILE_FLOATS:
        raise ValueError(f"resample: {rate_in} Hz -> {rate_out} Hz reads {o / n:.1f} input samples per output; a workgroup's input tile "
                         f"({plan.tile_floats()} floats) exceeds the {MAX_TILE_FLOATS} floats of LDS it may stage; convert through an "
                         f"intermediate rate")
    for a in (plan.first, plan.bank, plan.bank32):
        a.setflags(write=False)
    _plans[key] = plan
    return plan


# ---------------------------------------------------------------------------------------------- integer planning
def ready_outputs(plan: ResamplePlan, got: int) -> int:
    """how many outputs [0, m) of an open signal have all nt taps below `got`, the number of input samples known so far"""
    lo, hi = 0, ((int(got) + plan.width) // plan.o + 2) * plan.n              # pos(hi) + nt > got
    while lo < hi:
        mid = (lo + hi) // 2
        if plan.pos(mid) + plan.nt <= got:
            lo = mid + 1
        else:
            hi = mid
    return lo


def check_coverage(plan: ResamplePlan, in_start: int, in_count: int, out_start: int, out_count: int, total: Optional[int]) -> None:
    """every input sample that outputs [out_start, out_start + out_count) read inside [0, total) lies in the window
    [in_start, in_start + in_count); the kernel treats everything else as zero, so a sample not supplied would silently read as 0"""
    if out_count <= 0:
        return
    lo = max(0, plan.pos(out_start))
    hi = plan.pos(out_start + out_count - 1) + plan.nt
    if total is not None:
        if out_start + out_count > plan.out_len(total):
            raise ValueError(f"resample: outputs [{out_start}, {out_start + out_count}) lie beyond the {plan.out_len(total)} of a signal of {total} samples")
        hi = min(hi, int(total))
    if lo < hi and (lo < in_start or hi > in_start + in_count):
        raise ValueError(f"resample: outputs [{out_start}, {out_start + out_count}) read input samples [{lo}, {hi}), the window holds "
                         f"[{in_start}, {in_start + in_count})")


class ResampleStream:
    """Streaming state of one signal: push() takes consecutive chunks of input samples and returns every output sample whose taps are
    all known; the input tail later outputs still need is kept, and the rest comes out with ``final=True``.  Every output has the
    same taps in the same order as in a whole-signal run, so the chunks joined equal it bit for bit (as CodecStream)."""

    def __init__(self, plan: ResamplePlan, run: Callable[[np.ndarray, int, int, int, Optional[int]], np.ndarray]):
        self.plan, self.run = plan, run                         # run(window, in_start, out_start, out_count, total) -> float32 [out_count]
        self.buf = np.zeros(0, dtype=np.float32)                # samples [base, got)
        self.base = 0
        self.got = 0
        self.emitted = 0                                        # outputs handed out so far: the start offset of the next chunk
        self.final = False

    def push(self, chunk, final: bool = False) -> np.ndarray:
        if self.final:
            raise RuntimeError("ResampleStream: push() after the final chunk")
        c = np.asarray(chunk, dtype=np.float32).reshape(-1)
        self.buf = np.concatenate([self.buf, c])
        self.got += c.shape[0]
        self.final = bool(final)
        ready = self.plan.out_len(self.got) if final else max(self.emitted, ready_outputs(self.plan, self.got))
        parts = []
        step = max(1, (MAX_T - self.plan.nt - 2) * self.plan.n // max(self.plan.o, self.plan.n))
        while self.emitted < ready:                             # a launch takes at most MAX_T samples per row, in and out
            cnt = min(ready - self.emitted, step)
            lo = min(max(self.base, self.plan.pos(self.emitted)), self.got)
            hi = min(self.got, max(lo, self.plan.pos(self.emitted + cnt - 1) + self.plan.nt))
            parts.append(self.run(self.buf[lo - self.base:hi - self.base], lo, self.emitted, cnt, self.got if final else None))
            self.emitted += cnt
        keep = min(self.got, max(self.base, self.plan.pos(self.emitted)))       # earlier samples are never read again
        if keep > self.base:
            self.buf = self.buf[keep - self.base:].copy()
            self.base = keep
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


class _Identity:
    """the stream of equal rates: chunks pass through"""

    def __init__(self):
        self.emitted, self.final = 0, False

    def push(self, chunk, final: bool = False) -> np.ndarray:
        if self.final:
            raise RuntimeError("ResampleStream: push() after the final chunk")
        self.final = bool(final)
        c = np.asarray(chunk, dtype=np.float32).reshape(-1)
        self.emitted += c.shape[0]
        return c


# ---------------------------------------------------------------------------------------------- the device side
def _fn():
    return hb.lib().dia_resample


class DeviceResampler:
    """dia_resample on one HIP device: the plans' banks are uploaded once per rate pair (transposed, [nt][n]); every call goes host to
    device to host.  There is no CPU fallback."""

    def __init__(self, device=None):
        import torch

        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        _fn()
        self._banks: dict = {}

    def _bank(self, plan: ResamplePlan):
        import torch

        key = (plan.rate_in, plan.rate_out)
        if key not in self._banks:
            self._banks[key] = (torch.from_numpy(np.ascontiguousarray(plan.bank32.T)).to(self.device),
                                torch.from_numpy(np.array(plan.first)).to(self.device))      # a copy: the plan's arrays are read-only
        return self._banks[key]

    def launch(self, plan: ResamplePlan, x, y, in_start: Sequence[int], in_count: Sequence[int], out_start: Sequence[int],
               out_count: Sequence[int], total: Sequence[Optional[int]]) -> None:
        """one dia_resample launch on device tensors x fp32 [B, ldx] -> y fp32 [B, ldy], B <= MAX_ROWS; row b holds input samples
        [in_start[b], + in_count[b]) of a signal of total[b] samples (None: open) and receives outputs [out_start[b], + out_count[b])"""
        import torch

        B = x.shape[0]
        for b in range(B):
            check_coverage(plan, int(in_start[b]), int(in_count[b]), int(out_start[b]), int(out_count[b]), None if total[b] is None else int(total[b]))
        bank, first = self._bank(plan)
        a = hb.ResampleArgs(x=hb.ptr(x), y=hb.ptr(y), bank=hb.ptr(bank), first=hb.ptr(first), B=B, ldx=x.shape[1], ldy=y.shape[1],
                            o=plan.o, n=plan.n, nt=plan.nt,
                            in_start=(C.c_int64 * B)(*[int(v) for v in in_start]), out_start=(C.c_int64 * B)(*[int(v) for v in out_start]),
                            total=(C.c_int64 * B)(*[hb.RESAMPLE_OPEN if v is None else int(v) for v in total]),
                            in_count=(C.c_int32 * B)(*[int(v) for v in in_count]), out_count=(C.c_int32 * B)(*[int(v) for v in out_count]))
        with torch.cuda.device(self.device):
            hb.check(_fn()(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_resample")

    def run_rows(self, plan: ResamplePlan, buf: np.ndarray, in_start: Sequence[int], in_count: Sequence[int], out_start: Sequence[int],
                 out_count: Sequence[int], total: Sequence[Optional[int]]) -> List[np.ndarray]:
        """host rows buf [B, ld] (whatever lies beyond in_count[b] is never read) through launches of at most MAX_ROWS rows"""
        import torch

        buf = np.ascontiguousarray(buf, dtype=np.float32)
        out: List[np.ndarray] = []
        for g0 in range(0, buf.shape[0], MAX_ROWS):
            sl = slice(g0, min(buf.shape[0], g0 + MAX_ROWS))
            x = torch.from_numpy(buf[sl]).to(self.device)
            y = torch.empty(x.shape[0], max(1, max(out_count[sl])), dtype=torch.float32, device=self.device)
            self.launch(plan, x, y, in_start[sl], in_count[sl], out_start[sl], out_count[sl], total[sl])
            yh = y.cpu().numpy()
            out.extend(yh[r] if c == yh.shape[1] else yh[r, :c].copy() for r, c in enumerate(out_count[sl]))
        return out

    def resample_padded(self, buf: np.ndarray, lengths: Sequence[int], rate_in: int, rate_out: int) -> List[np.ndarray]:
        """rows of a 2-D buffer [B, ld], row b holding a whole signal of lengths[b] samples -> float32 [ceil(n lengths[b] / o)] each"""
        plan = resample_plan(rate_in, rate_out)
        buf = np.asarray(buf)
        lengths = [int(v) for v in lengths]
        if buf.ndim != 2 or len(lengths) != buf.shape[0] or any(v < 0 or v > buf.shape[1] for v in lengths):
            raise ValueError("resample: a buffer [B, ld] and one length in [0, ld] per row")
        if buf.shape[1] > MAX_T or plan.out_len(max(lengths + [0])) > MAX_T:
            raise ValueError(f"resample: more than {MAX_T} samples per row; use stream()")
        if buf.shape[1] == 0:
            return [np.zeros(0, dtype=np.float32) for _ in lengths]
        zero = [0] * len(lengths)
        return self.run_rows(plan, buf, zero, lengths, zero, [plan.out_len(v) for v in lengths], lengths)

    def resample(self, waves, rate_in: int, rate_out: int):
        """one mono float array [L], or a list of them with their own lengths (one launch), at rate_in -> float32 [ceil(n L / o)] at
        rate_out each.  Equal rates return the input unchanged."""
        if int(rate_in) == int(rate_out):
            return waves
        single = not isinstance(waves, (list, tuple))
        rows = []
        for w in ([waves] if single else waves):
            w = np.asarray(w.detach().cpu() if hasattr(w, "detach") else w)
            if w.ndim == 2 and w.shape[0] == 1:
                w = w[0]
            if w.ndim != 1 or w.dtype.kind != "f":
                raise ValueError(f"resample: a waveform of shape {tuple(w.shape)} and dtype {w.dtype}, expected mono float samples [L]")
            rows.append(w.astype(np.float32, copy=False))
        buf = np.empty((len(rows), max([r.shape[0] for r in rows] + [0])), dtype=np.float32)     # what lies behind a row is never read
        for b, r in enumerate(rows):
            buf[b, :r.shape[0]] = r
        out = self.resample_padded(buf, [r.shape[0] for r in rows], rate_in, rate_out)
        return out[0] if single else out

    def stream(self, rate_in: int, rate_out: int) -> Union[ResampleStream, "_Identity"]:
        """a streaming state for one signal on this device"""
        if int(rate_in) == int(rate_out):
            return _Identity()
        plan = resample_plan(rate_in, rate_out)

        def run(window: np.ndarray, in_start: int, out_start: int, out_count: int, total: Optional[int]) -> np.ndarray:
            buf = window[None] if window.shape[0] else np.zeros((1, 1), dtype=np.float32)
            return self.run_rows(plan, buf, [in_start], [window.shape[0]], [out_start], [out_count], [total])[0]

        return ResampleStream(plan, run)
