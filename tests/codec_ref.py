"""Plain-torch restatement of the DAC 44 kHz decode path (quantizer.from_codes, then decoder), the reference of every codec
comparison.  It takes a checkpoint-form state dict (weight_g / weight_v apart), folds weight norm itself and runs on the CPU in
the dtype asked for.  From dia_hip/codec.py it uses only the configuration class."""
import numpy as np
import torch
import torch.nn.functional as F


def fold(g, v, dtype):
    """w = g v / |v|, the norm over every dimension but 0 (for a transposed convolution dimension 0 is the input channel)"""
    v = v.to(torch.float64)
    dims = tuple(range(1, v.dim()))
    return (g.to(torch.float64) * v / v.pow(2).sum(dim=dims, keepdim=True).sqrt()).to(dtype)


def snake(x, alpha):
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


class RefCodec:
    def __init__(self, cfg, sd, dtype=torch.float64):
        self.cfg, self.dtype = cfg, dtype
        self.sd = sd
        self._w = {}

    def w(self, key):
        if key not in self._w:
            self._w[key] = fold(self.sd[key + ".weight_g"], self.sd[key + ".weight_v"], self.dtype)
        return self._w[key]

    def b(self, key):
        return self.sd[key + ".bias"].to(self.dtype)

    def alpha(self, key):
        return self.sd[key + ".alpha"].to(self.dtype)

    def from_codes(self, codes):
        """codes int64 [B, n_codebooks, T] -> z [B, latent, T]"""
        z = 0
        for i in range(self.cfg.n_codebooks):
            q = f"quantizer.quantizers.{i}"
            e = F.embedding(codes[:, i, :], self.sd[f"{q}.codebook.weight"].to(self.dtype)).transpose(1, 2)
            z = z + F.conv1d(e, self.w(f"{q}.out_proj"), self.b(f"{q}.out_proj"))
        return z

    def decoder(self, z):
        x = F.conv1d(z, self.w("decoder.model.0"), self.b("decoder.model.0"), padding=3)
        for i, s in enumerate(self.cfg.decoder_rates):
            blk = f"decoder.model.{i + 1}.block"
            x = snake(x, self.alpha(f"{blk}.0"))
            x = F.conv_transpose1d(x, self.w(f"{blk}.1"), self.b(f"{blk}.1"), stride=s, padding=-(-s // 2))
            for u, d in enumerate((1, 3, 9)):
                ru = f"{blk}.{2 + u}.block"
                y = snake(x, self.alpha(f"{ru}.0"))
                y = F.conv1d(y, self.w(f"{ru}.1"), self.b(f"{ru}.1"), dilation=d, padding=3 * d)
                y = snake(y, self.alpha(f"{ru}.2"))
                y = F.conv1d(y, self.w(f"{ru}.3"), self.b(f"{ru}.3"))
                x = x + y
        n = len(self.cfg.decoder_rates)
        x = snake(x, self.alpha(f"decoder.model.{n + 1}"))
        x = F.conv1d(x, self.w(f"decoder.model.{n + 2}"), self.b(f"decoder.model.{n + 2}"), padding=3)
        return torch.tanh(x)

    def decode(self, codes):
        """codes [n_codebooks, T] or [1, n_codebooks, T] (array or tensor) -> numpy [T * hop] in this codec's dtype"""
        c = torch.as_tensor(np.asarray(codes)).to(torch.int64)
        if c.dim() == 2:
            c = c[None]
        if c.shape[-1] == 0:
            return np.zeros(0, dtype=np.float64 if self.dtype == torch.float64 else np.float32)
        with torch.no_grad():
            return self.decoder(self.from_codes(c))[0, 0].numpy()


def random_codes(cfg, T, seed, B=None):
    """random ids that include 0 and codebook_size - 1"""
    g = np.random.default_rng(seed)
    shape = (cfg.n_codebooks, T) if B is None else (B, cfg.n_codebooks, T)
    c = g.integers(0, cfg.codebook_size, size=shape, dtype=np.int64)
    flat = c.reshape(-1)
    flat[0] = 0
    flat[-1] = cfg.codebook_size - 1
    return c
