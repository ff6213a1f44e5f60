"""Audio distance on the HIP device (csrc/spectral.hip, DESIGN.md "Audio distance"): the multi-scale STFT distance and the
multi-scale log-mel distance that the DAC paper evaluates on, between waveforms that are already where the codec and the resampler run.

The arithmetic is restated here from its formulas: the periodic Hann window, ``torch.stft(center=True, pad_mode="constant")``
framing at hop = window / 4, the Slaney-scale, Slaney-normalised triangular mel bank (fmin 0, fmax rate / 2), and the two L1 terms
    mag_term = mean |Sa - Sb|        log_term = mean |log10(max(Sa, eps)^p) - log10(max(Sb, eps)^p)|
over frames x bins (or frames x mels).  ``audiotools`` and ``librosa`` are not needed and the restatement is unpinned against them;
the defaults (STFT_DEFAULT, MEL_DEFAULT) are taken from the DAC paper's description of its evaluation and are unpinned too.

Host side only: the DFT basis and the filterbank in float64, rounded once to fp32 (spectral_plan), and the final float64 sum of the
kernel's per-tile partials in tile order.  All arithmetic on samples happens in the library (dia_spectral).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as hb

MAX_ROWS = 64                        # DIA_SPECTRAL_MAX_ROWS: row pairs of one launch
MAX_T = 1 << 24                      # DIA_SPECTRAL_MAX_T: samples per row
MIN_WINDOW, MAX_WINDOW = 32, 2048    # DIA_SPECTRAL_MIN_WINDOW / _MAX_WINDOW
MAX_MELS = 320                       # DIA_SPECTRAL_MAX_MELS
TILE_FRAMES = 16                     # DIA_SPECTRAL_TILE_FRAMES: frames of one partial
EPS = 1e-5

# a metric: sum over its resolutions of mag_weight * mag_term + log_weight * log_term, divided by their count
STFT_DEFAULT = dict(windows=(2048, 512), n_mels=None, mag_weight=1.0, log_weight=1.0, power=2)
MEL_DEFAULT = dict(windows=(32, 64, 128, 256, 512, 1024, 2048), n_mels=(5, 10, 20, 40, 80, 160, 320), mag_weight=0.0, log_weight=1.0, power=1)
METRICS = {"stft": STFT_DEFAULT, "mel": MEL_DEFAULT}


def hop_of(window: int) -> int:
    return int(window) // 4


def n_frames(length: int, window: int) -> int:
    return 1 + int(length) // hop_of(window)


def check_window(window: int) -> int:
    window = int(window)
    if window < MIN_WINDOW or window > MAX_WINDOW or window & (window - 1):
        raise ValueError(f"spectral: window = {window} is not a power of two in [{MIN_WINDOW}, {MAX_WINDOW}]")
    return window


def hz_to_mel(f):
    """the Slaney scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)"""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    with np.errstate(divide="ignore"):
        log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / math.log(6.4))
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (math.log(6.4) / 27.0)), m * 200.0 / 3.0)


def mel_filterbank(window: int, rate: int, n_mels: int) -> np.ndarray:
    """float64 [n_mels][window / 2 + 1]: triangles between n_mels + 2 points equally spaced in mel from 0 to rate / 2, each scaled
    by 2 / (its width in Hz).  A filter narrower than the bin spacing may contain no bin: its row is zero."""
    n_mels = int(n_mels)
    if n_mels < 1 or n_mels > MAX_MELS:
        raise ValueError(f"spectral: n_mels = {n_mels} outside [1, {MAX_MELS}]")
    if int(rate) < 1:
        raise ValueError(f"spectral: sample rate {rate} Hz must be positive")
    freqs = np.linspace(0.0, rate / 2.0, window // 2 + 1)
    pts = mel_to_hz(np.linspace(0.0, float(hz_to_mel(rate / 2.0)), n_mels + 2))
    width = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper))
    return fb * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def dft_basis(window: int) -> np.ndarray:
    """float64 [window][2][window / 2 + 1]: w[n] cos(2 pi n k / window) and -w[n] sin(2 pi n k / window), w the periodic Hann
    window; the angle is reduced exactly (n k mod window) before it is scaled"""
    n = np.arange(window, dtype=np.int64)
    k = np.arange(window // 2 + 1, dtype=np.int64)
    ang = ((n[:, None] * k[None, :]) % window).astype(np.float64) * (2.0 * math.pi / window)
    w = 0.5 - 0.5 * np.cos(2.0 * math.pi * n.astype(np.float64) / window)
    return np.stack([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)], axis=1)


@dataclass(frozen=True)
class SpectralPlan:
    window: int
    rate: Optional[int]
    n_mels: int                      # 0: magnitudes only
    basis32: np.ndarray              # float32 [window][2][nbin]
    fb32: Optional[np.ndarray]       # float32 [n_mels][nbin]
    fb_range: Optional[np.ndarray]   # int32 [n_mels][2]: the bins [lo, hi) that hold row m's nonzero weights (lo == hi: an empty filter)

    @property
    def nbin(self) -> int:
        return self.window // 2 + 1

    @property
    def hop(self) -> int:
        return self.window // 4

    @property
    def width(self) -> int:
        """values per frame of this plan's spectrum"""
        return self.n_mels or self.nbin


_plans: Dict[Tuple[int, Optional[int], int], SpectralPlan] = {}
_bases: Dict[int, np.ndarray] = {}


def spectral_plan(window: int, rate: Optional[int] = None, n_mels: Optional[int] = None) -> SpectralPlan:
    """the plan of one resolution, cached: the basis, and with n_mels the filterbank of `rate`; float64, rounded once to fp32"""
    window = check_window(window)
    n_mels = int(n_mels or 0)
    if n_mels and rate is None:
        raise ValueError("spectral: a mel plan needs the sample rate")
    key = (window, int(rate) if n_mels else None, n_mels)
    if key in _plans:
        return _plans[key]
    if window not in _bases:
        _bases[window] = dft_basis(window).astype(np.float32)
        _bases[window].setflags(write=False)
    fb32 = rng = None
    if n_mels:
        fb32 = mel_filterbank(window, int(rate), n_mels).astype(np.float32)
        nz = fb32 != 0
        lo = np.where(nz.any(axis=1), nz.argmax(axis=1), 0)
        hi = np.where(nz.any(axis=1), fb32.shape[1] - nz[:, ::-1].argmax(axis=1), 0)
        rng = np.ascontiguousarray(np.stack([lo, hi], axis=1).astype(np.int32))
        fb32.setflags(write=False)
        rng.setflags(write=False)
    plan = SpectralPlan(window, key[1], n_mels, _bases[window], fb32, rng)
    _plans[key] = plan
    return plan


def as_rows(waves, what: str = "spectral") -> Tuple[List[np.ndarray], bool]:
    """one mono float array [L] (or [1, L]), or a list of them -> (float32 rows, whether it was a single one)"""
    single = not isinstance(waves, (list, tuple))
    rows = []
    for w in ([waves] if single else waves):
        w = np.asarray(w.detach().cpu() if hasattr(w, "detach") else w)
        if w.ndim == 2 and w.shape[0] == 1:
            w = w[0]
        if w.ndim != 1 or w.dtype.kind != "f":
            raise ValueError(f"{what}: a waveform of shape {tuple(w.shape)} and dtype {w.dtype}, expected mono float samples [L]")
        if w.shape[0] < 1 or w.shape[0] > MAX_T:
            raise ValueError(f"{what}: a waveform of {w.shape[0]} samples, expected 1 .. {MAX_T}")
        rows.append(np.ascontiguousarray(w, dtype=np.float32))
    return rows, single


def pair_rows(a, b, trim: bool = False) -> Tuple[List[np.ndarray], List[np.ndarray], bool]:
    """the row pairs of a distance: as many rows in b as in a, pair by pair of equal length, or cut to the shorter with trim"""
    ra, single = as_rows(a, "spectral: a")
    rb, single_b = as_rows(b, "spectral: b")
    if len(ra) != len(rb) or single != single_b:
        raise ValueError(f"spectral: {len(ra)} waveforms against {len(rb)}")
    for i, (x, y) in enumerate(zip(ra, rb)):
        if x.shape[0] != y.shape[0]:
            if not trim:
                raise ValueError(f"spectral: pair {i} has {x.shape[0]} samples against {y.shape[0]}; pass trim=True to cut to the shorter")
            n = min(x.shape[0], y.shape[0])
            ra[i], rb[i] = x[:n], y[:n]
    return ra, rb, single


def metric_spec(name: str, override: Optional[dict]) -> dict:
    if name not in METRICS:
        raise ValueError(f"spectral: unknown metric {name!r}, expected one of {sorted(METRICS)}")
    spec = dict(METRICS[name])
    spec.update(override or {})
    spec["windows"] = tuple(int(w) for w in spec["windows"])
    if name == "mel":
        spec["n_mels"] = tuple(int(m) for m in spec["n_mels"])
        if len(spec["n_mels"]) != len(spec["windows"]):
            raise ValueError("spectral: the mel metric needs one n_mels per window")
    else:
        spec["n_mels"] = (0,) * len(spec["windows"])
    if not spec["windows"]:
        raise ValueError(f"spectral: metric {name!r} without a resolution")
    if spec["power"] not in (1, 2):
        raise ValueError(f"spectral: power = {spec['power']} is neither 1 nor 2")
    return spec


def _fn():
    return hb.lib().dia_spectral


class DeviceSpectral:
    """dia_spectral on one HIP device: the plans' bases and filterbanks are uploaded once per resolution; every call goes host to
    device to host.  There is no CPU fallback."""

    def __init__(self, device=None):
        import torch

        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise hb.DiaHipError(f"device {self.device} is not a HIP device; there is no CPU fallback")
        _fn()
        self._dev: dict = {}

    def _plan(self, plan: SpectralPlan):
        import torch

        key = (plan.window, plan.rate, plan.n_mels)
        if key not in self._dev:
            if ("basis", plan.window) not in self._dev:
                self._dev[("basis", plan.window)] = torch.from_numpy(np.array(plan.basis32)).to(self.device)   # copies: the plan's arrays are read-only
            fb = torch.from_numpy(np.array(plan.fb32)).to(self.device) if plan.n_mels else None
            rng = torch.from_numpy(np.array(plan.fb_range)).to(self.device) if plan.n_mels else None
            self._dev[key] = (self._dev[("basis", plan.window)], fb, rng)
        return self._dev[key]

    def _upload(self, rows: Sequence[np.ndarray]):
        import torch

        buf = np.zeros((len(rows), max(r.shape[0] for r in rows)), dtype=np.float32)
        for i, r in enumerate(rows):
            buf[i, :r.shape[0]] = r
        return torch.from_numpy(buf).to(self.device)

    def launch(self, plan: SpectralPlan, a, b, lengths: Sequence[int], *, partial=None, out=None, power: int = 1, eps: float = EPS) -> None:
        """one dia_spectral launch on device tensors a (and b) fp32 [B, ld], B <= MAX_ROWS: into partial float64 [B, tiles, 2] with
        b, into out fp32 [B, out_frames, plan.width] without"""
        import torch

        basis, fb, rng = self._plan(plan)
        B = a.shape[0]
        args = hb.SpectralArgs(a=hb.ptr(a), b=hb.ptr(b), basis=hb.ptr(basis), fb=hb.ptr(fb), fb_range=hb.ptr(rng),
                               partial=hb.ptr(partial), out=hb.ptr(out), B=B, ld=a.shape[1], window=plan.window, n_mels=plan.n_mels,
                               tiles=0 if partial is None else partial.shape[1], out_frames=0 if out is None else out.shape[1],
                               power=int(power), eps=float(eps), len=(C.c_int32 * B)(*[int(v) for v in lengths]))
        with torch.cuda.device(self.device):
            hb.check(_fn()(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dia_spectral")

    def _spectra(self, waves, plan: SpectralPlan):
        import torch

        rows, single = as_rows(waves)
        res: List[np.ndarray] = []
        for g0 in range(0, len(rows), MAX_ROWS):
            grp = rows[g0:g0 + MAX_ROWS]
            lens = [r.shape[0] for r in grp]
            frames = [n_frames(n, plan.window) for n in lens]
            out = torch.empty(len(grp), max(frames), plan.width, dtype=torch.float32, device=self.device)
            self.launch(plan, self._upload(grp), None, lens, out=out)
            host = out.cpu().numpy()
            res.extend(host[i, :f].copy() for i, f in enumerate(frames))
        return res[0] if single else res

    def stft_mag(self, waves, window: int):
        """|STFT| of one waveform or a list of them: float32 [1 + L // hop, window / 2 + 1] each"""
        return self._spectra(waves, spectral_plan(window))

    def logmel(self, waves, window: int, n_mels: int, rate: int, eps: float = EPS):
        """log10(max(mel, eps)) of one waveform or a list of them: float32 [1 + L // hop, n_mels] each.  The mel rows come from the
        device; the clamp and the logarithm are taken here, on the host"""
        mel = self._spectra(waves, spectral_plan(window, rate, n_mels))
        log = lambda m: np.log10(np.maximum(m, np.float32(eps)))
        return log(mel) if isinstance(mel, np.ndarray) else [log(m) for m in mel]

    def mel(self, waves, window: int, n_mels: int, rate: int):
        """the mel rows themselves: float32 [1 + L // hop, n_mels] each"""
        return self._spectra(waves, spectral_plan(window, rate, n_mels))

    def distance(self, a, b, rate: int, metrics: Sequence[str] = ("stft", "mel"), trim: bool = False, *, stft: Optional[dict] = None,
                 mel: Optional[dict] = None, eps: float = EPS):
        """the distances between waveform a and waveform b (or lists of them, pair by pair): per pair
        ``{"stft": x, "mel": y, "per_resolution": {metric: {window: {"mag": mag_term, "log": log_term}}}}``.  Pairs of unequal length
        raise unless trim=True, which cuts to the shorter.  `stft` / `mel` override entries of STFT_DEFAULT / MEL_DEFAULT."""
        import torch

        ra, rb, single = pair_rows(a, b, trim)
        specs = {name: metric_spec(name, {"stft": stft, "mel": mel}.get(name)) for name in metrics}
        plans = {(name, w): spectral_plan(w, rate, m) for name, s in specs.items() for w, m in zip(s["windows"], s["n_mels"])}
        res: List[dict] = []
        for g0 in range(0, len(ra), MAX_ROWS):
            ga, gb = ra[g0:g0 + MAX_ROWS], rb[g0:g0 + MAX_ROWS]
            lens = [r.shape[0] for r in ga]
            da, db = self._upload(ga), self._upload(gb)
            parts = {}
            for (name, w), plan in plans.items():               # every launch first, one download per resolution after the last
                tiles = -(-n_frames(max(lens), w) // TILE_FRAMES)
                parts[(name, w)] = torch.zeros(len(ga), tiles, 2, dtype=torch.float64, device=self.device)
                self.launch(plan, da, db, lens, partial=parts[(name, w)], power=specs[name]["power"], eps=eps)
            host = {k: v.cpu().numpy() for k, v in parts.items()}
            for i, n in enumerate(lens):
                row = {"per_resolution": {}}
                for name, s in specs.items():
                    total, per = 0.0, {}
                    for w in s["windows"]:
                        plan = plans[(name, w)]
                        F = n_frames(n, w)
                        # float64, in tile order: a running sum adds one tile after the other
                        sums = [float(v) for v in np.cumsum(host[(name, w)][i, :-(-F // TILE_FRAMES)], axis=0)[-1]]
                        per[w] = {"mag": sums[0] / (F * plan.width), "log": sums[1] / (F * plan.width)}
                        total += s["mag_weight"] * per[w]["mag"] + s["log_weight"] * per[w]["log"]
                    row[name] = total / len(s["windows"])
                    row["per_resolution"][name] = per
                res.append(row)
        return res[0] if single else res
