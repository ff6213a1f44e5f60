"""Loudness on the HIP device (csrc/loudness.hip, DESIGN.md "Loudness"): an ITU-R BS.1770-4 integrated-loudness meter for mono
signals (what EBU R 128 asks for), the true peak (4 x oversampled through the library's own 1 -> 4 resampling bank), and
normalisation to a target in LUFS under a true-peak ceiling.  normalize() is a PURE GAIN, not a limiter: where the target would
push the true peak over the ceiling, the whole row gets the smaller gain and ends below the target (the report says `limited`).

Host side only: the K-weighting coefficients in float64 (the libebur128 derivation, which gives the standard's 48 kHz table), the
chunk grid and the transition matrices the device's carry needs, the gating in float64 from the device's step sums, the gain rule
and the trim.  All arithmetic on samples happens in the library (dia_loudness).  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as hb
from .resample import resample_plan

MAX_ROWS = 64                        # DIA_LOUD_MAX_ROWS: rows of one launch
MAX_T = 1 << 24                      # DIA_LOUD_MAX_T: samples per row of one launch
MIN_STEP, MAX_STEP = 8, 19200        # DIA_LOUD_MIN_STEP / DIA_LOUD_MAX_STEP
MAX_CHUNKS = 64                      # DIA_LOUD_MAX_CHUNKS: one lane per chunk of a step
MIN_CHUNK = 64                       # below this the carry over the chunks costs more than the chunks
ABSOLUTE_GATE = -70.0                # LKFS
RELATIVE_GATE = -10.0                # LU below the mean of the absolutely gated blocks
BLOCK_STEPS = 4                      # a 400 ms block is four 100 ms steps; blocks overlap by three
OFFSET = -0.691

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)     # f0, gain in dB, Q
HIGHPASS = (38.13547087602444, 0.5003270373238773)                     # f0, Q


def k_weighting(rate: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> (shelf b [3], shelf a [3], high-pass b [3], high-pass a [3]) in float64 for `rate`; at 48 kHz the table of BS.1770"""
    fs = float(rate)
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], dtype=np.float64)
    sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hb_ = np.array([1.0, -2.0, 1.0], dtype=np.float64)
    ha = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    return sb, sa, hb_, ha


def _advance(s: Sequence[float], x: float, c: Sequence[float]) -> Tuple[List[float], float]:
    """one sample through the cascade (transposed direct form II): state (s1, s2 of the shelf, s1, s2 of the high-pass),
    c = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 -> (new state, output)"""
    y1 = c[0] * x + s[0]
    a = [c[1] * x + s[1] - c[3] * y1, c[2] * x - c[4] * y1]
    y2 = c[5] * y1 + s[2]
    return a + [c[6] * y1 + s[3] - c[8] * y2, c[7] * y1 - c[9] * y2], y2


def choose_chunk(step: int) -> int:
    """samples of a chunk.  At least MIN_CHUNK and step / MAX_CHUNKS, and ODD, so that the 64 lanes of a wave, which read LDS at a
    stride of one chunk, hit 64 banks; an odd divisor of the step within a factor of two is preferred (no short last chunk)."""
    lo = max(MIN_CHUNK, -(-step // MAX_CHUNKS))
    if step <= lo:
        return step
    lo |= 1
    for c in range(lo, min(2 * lo, step + 1), 2):
        if step % c == 0:
            return c
    return lo


class LoudnessPlan:
    """one sample rate: the K-weighting, the 100 ms step and 400 ms block in samples, and the chunk grid of the device's parallel
    recursion: chunk k of step s covers samples [s * step + k * chunk, min(.. + chunk, (s + 1) * step)), so no chunk straddles a
    step.  `table` is what dia_loudness reads (the layout is in include/dia_hip.h)."""

    def __init__(self, rate: int):
        if isinstance(rate, bool) or int(rate) != rate:
            raise ValueError(f"loudness: sample rate {rate!r} is not an integer")
        self.rate = int(rate)
        self.step = (self.rate + 5) // 10                       # round(rate / 10), halves up (as libebur128)
        if self.step < MIN_STEP or self.step > MAX_STEP:
            raise ValueError(f"loudness: sample rate {rate} Hz outside [{MIN_STEP * 10 - 5}, {MAX_STEP * 10 + 4}]")
        self.block = BLOCK_STEPS * self.step
        self.chunk = choose_chunk(self.step)
        self.chunks = -(-self.step // self.chunk)
        sb, sa, hb_, ha = k_weighting(self.rate)
        self.shelf_b, self.shelf_a, self.hp_b, self.hp_a = sb, sa, hb_, ha
        self.coef = np.array([sb[0], sb[1], sb[2], sa[1], sa[2], hb_[0], hb_[1], hb_[2], ha[1], ha[2]], dtype=np.float64)
        c = [float(v) for v in self.coef]
        eye = np.eye(4)
        self.A = np.array([_advance(list(eye[k]), 0.0, c)[0] for k in range(4)], dtype=np.float64).T        # column k: A e_k
        mp = np.linalg.matrix_power
        self.table = np.concatenate([self.coef, mp(self.A, self.chunk).reshape(-1), mp(self.A, self.step).reshape(-1)]
                                    + [mp(self.A, k * self.chunk).reshape(-1) for k in range(self.chunks)])
        up = resample_plan(1, 4)                                # the true-peak oversampler: the library's own bank
        self.nt, self.first, self.bank32 = up.nt, up.first, up.bank32

    def chunk_bounds(self, n: int) -> List[Tuple[int, int]]:
        """[lo, hi) of every chunk of the whole steps of a row of n samples"""
        out = []
        for s in range(int(n) // self.step):
            for k in range(self.chunks):
                lo = s * self.step + k * self.chunk
                out.append((lo, min(lo + self.chunk, (s + 1) * self.step)))
        return out


_plans: Dict[int, LoudnessPlan] = {}


def loudness_plan(rate: int) -> LoudnessPlan:
    if rate not in _plans:
        _plans[rate] = LoudnessPlan(rate)
    return _plans[rate]


# ---------------------------------------------------------------------------------------------- gating, gain and trim (float64)
def _lk(z: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(z)


def integrated(steps, step: int) -> float:
    """BS.1770-4 gating over the float64 sums of squares of a row's whole steps: 400 ms blocks from four consecutive steps (75 %
    overlap), the absolute gate at -70 LKFS, the relative gate 10 LU below the mean of the absolutely gated blocks.  -inf for a row
    shorter than one block or with every block gated."""
    s = np.asarray(steps, dtype=np.float64).reshape(-1)
    if s.shape[0] < BLOCK_STEPS:
        return -math.inf
    z = (s[:-3] + s[1:-2] + s[2:-1] + s[3:]) / float(BLOCK_STEPS * int(step))
    l = _lk(z)
    keep = l >= ABSOLUTE_GATE
    if not keep.any():
        return -math.inf
    rel = float(_lk(np.mean(z[keep]))) + RELATIVE_GATE
    keep &= l > rel
    if not keep.any():
        return -math.inf
    return float(_lk(np.mean(z[keep])))


def db(v: float) -> float:
    """20 log10 of a linear peak; -inf for 0"""
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def choose_gain(loudness: float, true_peak_db: float, target: float, peak: float) -> Tuple[float, bool]:
    """-> (gain in dB, limited): target - loudness, lowered to peak - true_peak where it would cross the ceiling.  A row that
    measures -inf gets 0 dB."""
    if not math.isfinite(loudness):
        return 0.0, False
    g = float(target) - loudness
    if math.isfinite(true_peak_db) and true_peak_db + g > float(peak):
        return float(peak) - true_peak_db, True
    return g, False


def trim_bounds(steps, step: int, n: int, trim_db: Optional[float], trim_pad: int = 1) -> Tuple[int, int]:
    """[start, stop) of the samples that stay: leading and trailing WHOLE steps whose own K-weighted loudness
    -0.691 + 10 log10(sum / step) is below trim_db go, except trim_pad of them on either side.  The samples behind the last whole
    step go with a dropped trailing step and stay otherwise.  Nothing goes when every step is that quiet."""
    n = int(n)
    if trim_db is None:
        return 0, n
    if trim_pad < 0:
        raise ValueError(f"loudness: trim_pad = {trim_pad} is negative")
    s = np.asarray(steps, dtype=np.float64).reshape(-1)
    loud = np.flatnonzero(_lk(s / float(step)) >= float(trim_db))
    if loud.shape[0] == 0:
        return 0, n
    lead, trail = int(loud[0]), s.shape[0] - 1 - int(loud[-1])
    start = max(0, lead - int(trim_pad)) * int(step)
    stop = n if trail <= trim_pad else (s.shape[0] - (trail - int(trim_pad))) * int(step)
    return start, stop


def as_rows(waves, what: str = "loudness"):
    """time_scale's input rules: one mono float array [N] (or [1, N]), or a list of them -> (single, [(given, float array)])"""
    single = not isinstance(waves, (list, tuple))
    rows = []
    for w in ([waves] if single else waves):
        a = np.asarray(w.detach().cpu() if hasattr(w, "detach") else w)
        if a.ndim == 2 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 1 or a.dtype.kind != "f":
            raise ValueError(f"{what}: a waveform of shape {tuple(a.shape)} and dtype {a.dtype}, expected mono float samples [N]")
        if a.shape[0] > MAX_T:
            raise ValueError(f"{what}: more than {MAX_T} samples in a row")
        rows.append((w, a))
    return single, rows


# ---------------------------------------------------------------------------------------------- the device side
def _fn():
    return hb.lib().dia_loudness


def _i32(v: Sequence[int]):
    return (C.c_int32 * len(v))(*[int(u) for u in v])


def ws_doubles(B: int, ld_steps: int, chunks: int) -> int:
    """DIA_LOUD_WS_DOUBLES"""
    return B * (ld_steps * (8 + 4 * chunks) + ld_steps + 1)


class DeviceLoudness:
    """dia_loudness on one HIP device: a rate's table and the oversampling bank are uploaded once; every call goes host to device to
    host.  There is no CPU fallback."""

    def __init__(self, device=None):
        import torch

        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        _fn()
        self._tables: dict = {}

    def _table(self, plan: LoudnessPlan):
        import torch

        if plan.rate not in self._tables:
            self._tables[plan.rate] = (torch.from_numpy(plan.table.copy()).to(self.device),
                                       torch.from_numpy(np.array(plan.bank32, dtype=np.float32)).to(self.device))
        return self._tables[plan.rate]

    def _call(self, a: "hb.LoudnessArgs") -> None:
        import torch

        with torch.cuda.device(self.device):
            hb.check(_fn()(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_loudness")

    def launch_measure(self, plan: LoudnessPlan, x, lens, steps, peaks, ws) -> None:
        """one DIA_LOUD_MEASURE launch on device tensors: x fp32 [B, ldx] with lens[b] samples each, B <= MAX_ROWS -> steps float64
        [B, ld_steps], peaks fp32 [B, 2]; ws float64, at least ws_doubles(B, ld_steps, plan.chunks)"""
        table, bank = self._table(plan)
        self._call(hb.LoudnessArgs(x=hb.ptr(x), steps=hb.ptr(steps), peaks=hb.ptr(peaks), ws=hb.ptr(ws), table=hb.ptr(table),
                                   bank=hb.ptr(bank), ws_doubles=ws.numel(), mode=hb.LOUD_MEASURE, B=x.shape[0], ldx=x.shape[1],
                                   ld_steps=steps.shape[1], step=plan.step, chunk=plan.chunk, chunks=plan.chunks, nt=plan.nt,
                                   first=_i32(plan.first), len=_i32(lens)))

    def launch_apply(self, x, y, lens, in_off, out_count, gain) -> None:
        """one DIA_LOUD_APPLY launch on device tensors: y[b, i] = float(double(x[b, in_off[b] + i]) * gain[b]), i < out_count[b]"""
        self._call(hb.LoudnessArgs(x=hb.ptr(x), y=hb.ptr(y), mode=hb.LOUD_APPLY, B=x.shape[0], ldx=x.shape[1], ldy=y.shape[1],
                                   len=_i32(lens), in_off=_i32(in_off), out_count=_i32(out_count),
                                   gain=(C.c_double * len(gain))(*[float(g) for g in gain])))

    @staticmethod
    def _pack(arrs: List[np.ndarray]) -> np.ndarray:
        buf = np.zeros((len(arrs), max(1, max(a.shape[0] for a in arrs))), dtype=np.float32)
        for b, a in enumerate(arrs):
            buf[b, :a.shape[0]] = a
        return buf

    def measure_rows(self, plan: LoudnessPlan, arrs: List[np.ndarray]) -> List[dict]:
        import torch

        out: List[dict] = []
        for g0 in range(0, len(arrs), MAX_ROWS):
            grp = arrs[g0:g0 + MAX_ROWS]
            lens = [a.shape[0] for a in grp]
            x = torch.from_numpy(self._pack(grp)).to(self.device)
            B, ld = len(grp), max(1, max(lens) // plan.step)
            steps = torch.zeros(B, ld, dtype=torch.float64, device=self.device)
            peaks = torch.zeros(B, 2, dtype=torch.float32, device=self.device)
            ws = torch.empty(ws_doubles(B, ld, plan.chunks), dtype=torch.float64, device=self.device)
            self.launch_measure(plan, x, lens, steps, peaks, ws)
            sh, ph = steps.cpu().numpy(), peaks.cpu().numpy()
            for b, n in enumerate(lens):
                s = sh[b, :n // plan.step].copy()
                out.append({"loudness": integrated(s, plan.step), "true_peak": db(float(ph[b, 1])), "sample_peak": db(float(ph[b, 0])),
                            "steps": s})
        return out

    def apply_rows(self, arrs: List[np.ndarray], in_off: Sequence[int], out_count: Sequence[int], gain: Sequence[float]) -> List[np.ndarray]:
        import torch

        out: List[np.ndarray] = []
        for g0 in range(0, len(arrs), MAX_ROWS):
            sl = slice(g0, g0 + MAX_ROWS)
            grp, cnt = arrs[sl], list(out_count[sl])
            x = torch.from_numpy(self._pack(grp)).to(self.device)
            y = torch.empty(len(grp), max(1, max(cnt)), dtype=torch.float32, device=self.device)
            self.launch_apply(x, y, [a.shape[0] for a in grp], in_off[sl], cnt, gain[sl])
            yh = y.cpu().numpy()
            out.extend(yh[b, :c].copy() for b, c in enumerate(cnt))
        return out

    def measure(self, waves, rate: int):
        """one mono float array [N], or a list of them with their own lengths (one launch per MAX_ROWS rows) -> per row
        {"loudness": LUFS (integrated, BS.1770-4; -inf below one 400 ms block or with every block gated), "true_peak": dBTP,
        "sample_peak": dBFS, "steps": float64 sums of squares of the K-weighted signal over the row's whole 100 ms steps}"""
        plan = loudness_plan(rate)
        single, rows = as_rows(waves)
        rep = self.measure_rows(plan, [a.astype(np.float32, copy=False) for _, a in rows]) if rows else []
        return rep[0] if single else rep

    def normalize(self, waves, rate: int, target: float = -23.0, peak: float = -1.0, trim_db: Optional[float] = None, trim_pad: int = 1):
        """-> (waves, reports).  Every row gets the gain target - loudness, lowered to peak - true_peak where it would push the true
        peak over the ceiling `peak` (dBTP): a pure gain, NOT a limiter, so a limited row ends below the target.  The report is
        measure()'s (of the input) plus "gain_db", "limited" and "kept" = [start, stop).  A row that measures -inf comes back
        unchanged with gain_db 0.  trim_db: leading and trailing whole steps quieter than that go, except trim_pad on either side
        (trim_bounds); the loudness is measured before the trim, and the same launch cuts and scales."""
        if not (math.isfinite(float(target)) and math.isfinite(float(peak))):
            raise ValueError(f"loudness: target = {target} / peak = {peak} is not finite")
        if trim_db is not None and math.isnan(float(trim_db)):
            raise ValueError("loudness: trim_db is not a number")
        if trim_pad < 0:
            raise ValueError(f"loudness: trim_pad = {trim_pad} is negative")
        plan = loudness_plan(rate)
        single, rows = as_rows(waves)
        arrs = [a.astype(np.float32, copy=False) for _, a in rows]
        rep = self.measure_rows(plan, arrs) if rows else []
        out: list = [w for w, _ in rows]
        at, off, cnt, gains = [], [], [], []
        for i, r in enumerate(rep):
            n = arrs[i].shape[0]
            r["gain_db"], r["limited"] = choose_gain(r["loudness"], r["true_peak"], target, peak)
            start, stop = (0, n) if not math.isfinite(r["loudness"]) else trim_bounds(r["steps"], plan.step, n, trim_db, trim_pad)
            r["kept"] = [start, stop]
            if math.isfinite(r["loudness"]):
                at.append(i); off.append(start); cnt.append(stop - start); gains.append(10.0 ** (r["gain_db"] / 20.0))
        if at:
            ys = self.apply_rows([arrs[i] for i in at], off, cnt, gains)
            for i, y in zip(at, ys):
                out[i] = y
        return (out[0], rep[0]) if single else (out, rep)

    def gain(self, waves, gain_db: float):
        """a fixed gain in dB on every row: float32(float64(x) * 10 ** (gain_db / 20))"""
        if not math.isfinite(float(gain_db)):
            raise ValueError(f"loudness: gain_db = {gain_db} is not finite")
        single, rows = as_rows(waves)
        arrs = [a.astype(np.float32, copy=False) for _, a in rows]
        at = [i for i, a in enumerate(arrs) if a.shape[0]]
        out: list = [a for a in arrs]
        if at:
            ys = self.apply_rows([arrs[i] for i in at], [0] * len(at), [arrs[i].shape[0] for i in at],
                                 [10.0 ** (float(gain_db) / 20.0)] * len(at))
            for i, y in zip(at, ys):
                out[i] = y
        return out[0] if single else out
