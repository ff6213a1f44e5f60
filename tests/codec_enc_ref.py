"""Plain-torch restatement of the DAC 44 kHz encode path (preprocess, encoder, the residual VQ search of quantizer.forward), the
reference of every encode-side comparison.  It follows DAC's expressions literally -- F.normalize of encodings and codebook, the
three-term distance, z_e + (z_q - z_e) -- takes a checkpoint-form state dict (decode and encode side together), folds weight norm
itself and runs on the CPU in the dtype asked for.  The arg-min takes the LOWEST index among equal distances, the library's rule.
Beside the codes it returns, per stage and frame, the margin (second-smallest distance minus the smallest) and the distances.
The restatement uses only the configuration class of dia_hip/codec.py; the case builders at the end (shared by the CPU and GPU
test files, so that the seeds checked on the CPU are the ones run on the device) also draw its synthetic weights."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from codec_ref import fold, snake


class RefEncoder:
    def __init__(self, cfg, sd, dtype=torch.float64):
        self.cfg, self.dtype, self.sd = cfg, dtype, sd
        self._w = {}

    def w(self, key):
        if key not in self._w:
            self._w[key] = fold(self.sd[key + ".weight_g"], self.sd[key + ".weight_v"], self.dtype)
        return self._w[key]

    def b(self, key):
        return self.sd[key + ".bias"].to(self.dtype)

    def alpha(self, key):
        return self.sd[key + ".alpha"].to(self.dtype)

    def preprocess(self, wave):
        """samples [L] -> [1, 1, L'] with zeros on the right up to a multiple of the hop"""
        x = torch.as_tensor(np.asarray(wave, dtype=np.float32)).reshape(1, 1, -1)
        return F.pad(x, (0, -x.shape[-1] % self.cfg.hop)).to(self.dtype)

    def encoder(self, x):
        """[B, 1, L] -> latent [B, latent, L / hop]"""
        x = F.conv1d(x, self.w("encoder.block.0"), self.b("encoder.block.0"), padding=3)
        for i, s in enumerate(self.cfg.encoder_rates):
            blk = f"encoder.block.{i + 1}.block"
            for u, d in enumerate((1, 3, 9)):
                ru = f"{blk}.{u}.block"
                y = snake(x, self.alpha(f"{ru}.0"))
                y = F.conv1d(y, self.w(f"{ru}.1"), self.b(f"{ru}.1"), dilation=d, padding=3 * d)
                y = snake(y, self.alpha(f"{ru}.2"))
                y = F.conv1d(y, self.w(f"{ru}.3"), self.b(f"{ru}.3"))
                x = x + y
            x = snake(x, self.alpha(f"{blk}.3"))
            x = F.conv1d(x, self.w(f"{blk}.4"), self.b(f"{blk}.4"), stride=s, padding=-(-s // 2))
        n = len(self.cfg.encoder_rates)
        x = snake(x, self.alpha(f"encoder.block.{n + 1}"))
        return F.conv1d(x, self.w(f"encoder.block.{n + 2}"), self.b(f"encoder.block.{n + 2}"), padding=1)

    def quantize(self, z):
        """latent [B, latent, T] -> (codes int64 [B, n, T], margins [B, n, T], distances [n][B T, codebook_size])"""
        B, _, T = z.shape
        residual, codes, margins, dists = z.to(self.dtype), [], [], []
        for i in range(self.cfg.n_codebooks):
            q = f"quantizer.quantizers.{i}"
            z_e = F.conv1d(residual, self.w(f"{q}.in_proj"), self.b(f"{q}.in_proj"))
            codebook = self.sd[f"{q}.codebook.weight"].to(self.dtype)
            enc = F.normalize(z_e.transpose(1, 2).reshape(B * T, -1))
            cb = F.normalize(codebook)
            dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
            two = torch.topk(dist, 2, dim=1, largest=False).values if dist.shape[1] > 1 else torch.cat([dist, dist + np.inf], 1)
            idx = (dist == two[:, :1]).to(torch.int8).argmax(dim=1)              # the first, i.e. lowest, index at the minimum
            z_q = F.embedding(idx.view(B, T), codebook).transpose(1, 2)
            z_q = z_e + (z_q - z_e)
            z_q = F.conv1d(z_q, self.w(f"{q}.out_proj"), self.b(f"{q}.out_proj"))
            residual = residual - z_q
            codes.append(idx.view(B, T))
            margins.append((two[:, 1] - two[:, 0]).view(B, T))
            dists.append(dist)
        return torch.stack(codes, 1), torch.stack(margins, 1), dists

    def latents(self, wave):
        """samples [L] -> numpy latent [latent, ceil(L / hop)] in this dtype"""
        if np.asarray(wave).shape[-1] == 0:
            return np.zeros((self.cfg.latent_dim, 0))
        with torch.no_grad():
            return self.encoder(self.preprocess(wave))[0].numpy()

    def encode(self, wave):
        """samples [L] -> (codes [n, T], latent [latent, T], margins [n, T], distances) as numpy arrays / a list of tensors"""
        with torch.no_grad():
            z = self.encoder(self.preprocess(wave))
            c, m, d = self.quantize(z)
        return c[0].numpy(), z[0].numpy(), m[0].numpy(), d


def make_wave(L, seed):
    """a waveform of RMS ~ 0.2: three partials that drift, plus noise, with a silent stretch at the start"""
    g = np.random.default_rng(seed)
    t = np.arange(L) / 44100.0
    f = g.uniform(90.0, 2500.0, size=3)
    x = sum(a * np.sin(2 * np.pi * (fi * t + 40.0 * np.sin(2 * np.pi * 1.5 * t + p))) for a, fi, p in zip((0.2, 0.12, 0.08), f, g.uniform(0, 6, 3)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t)) + 0.05 * g.standard_normal(L)
    x[:min(L, 64)] = 0.0
    return x.astype(np.float32)


def distance_error(d_lo, c_lo, d_hi, c_hi):
    """largest |distance of the low-precision run - float64's| over the (frame, stage) pairs both runs reach on the same path:
    a frame counts up to and including the first stage where the two runs chose differently"""
    same = np.ones(c_hi.shape[1], dtype=bool)
    worst = 0.0
    for i in range(c_hi.shape[0]):
        if same.any():
            diff = (d_lo[i].double() - d_hi[i].double()).abs().max(dim=1).values.numpy()
            worst = max(worst, float(diff[same].max()))
        same &= c_lo[i] == c_hi[i]
    return worst


def compare_codes(name, got, ref, margins, tau, cap):
    """the acceptance rule: `got` must equal `ref` [n, T] except at a (stage, frame) whose float64 margin is below tau; a frame is
    compared up to its first excused stage and dropped after it.  Returns the excused frames; more than `cap` of them fail."""
    excused = 0
    for t in range(ref.shape[1]):
        for i in range(ref.shape[0]):
            if got[i, t] == ref[i, t]:
                continue
            assert margins[i, t] < tau, f"{name}: frame {t} stage {i}: {got[i, t]} != {ref[i, t]} at margin {margins[i, t]:.3e} >= tau {tau:.3e}"
            excused += 1
            break
    print(f"codec-encode {name}: {excused} of {ref.shape[1]} frames excused (tau {tau:.3e}, cap {cap})")
    assert excused <= cap, (name, excused, cap)
    return excused


# ---------------------------------------------------------------------------------------------- shared cases
# (latent, T, seed) of the quantiser-alone cases.  tests/test_codec_encode_cpu.py runs the float32 restatement through the
# acceptance rule on exactly these and finds no excused frame in any of them.
QUANT_CASES = [(64, 1, 11), (64, 17, 12), (64, 130, 13), (1024, 1, 21), (1024, 17, 22), (1024, 130, 23)]


def whole_state(cfg, seed):
    from dia_hip import codec as K
    return {**K.synthetic_state_dict(cfg, seed), **K.synthetic_encoder_state(cfg, seed)}


@functools.lru_cache(maxsize=None)
def quant_case(latent, T, seed):
    """-> (cfg, state dict, latent fp32 [1, latent, T] = the float64 latent rounded, (codes, margins, distances) in float64,
    the same in float32), all on the rounded latent.  The encoder in front is the narrow one whatever the latent."""
    from dia_hip import codec as K
    cfg = K.CodecConfig(latent_dim=latent, decoder_dim=192, encoder_dim=8)
    sd = whole_state(cfg, seed)
    r64, r32 = RefEncoder(cfg, sd, torch.float64), RefEncoder(cfg, sd, torch.float32)
    with torch.no_grad():
        z = r64.encoder(r64.preprocess(make_wave(T * cfg.hop, seed))).float()
        c64, m64, d64 = r64.quantize(z.double())
        c32, m32, d32 = r32.quantize(z)
    return cfg, sd, z, (c64[0].numpy(), m64[0].numpy(), d64), (c32[0].numpy(), m32[0].numpy(), d32)


def latent_landing_on(ref, row):
    """a latent [1, latent, 1] (fp32 values) whose stage-0 projection points along codebook row `row`"""
    q = "quantizer.quantizers.0"
    W = ref.w(f"{q}.in_proj")[:, :, 0].double()
    target = 3.0 * ref.sd[f"{q}.codebook.weight"][row].double() - ref.b(f"{q}.in_proj").double()
    z = torch.linalg.pinv(W) @ target
    return z.float().to(ref.dtype).reshape(1, -1, 1)
