"""Float64 restatements for the codec's bf16 modes (csrc/codec_bf16.hip, DESIGN.md "Codec: bf16 modes"): the device's plane split,
an emulation of the whole decoder with every convolution operand split that way, the derived bound of the fp32 accumulation, and
inputs whose Snake value is clear of the hi plane's rounding boundaries.  From dia_hip/codec.py it uses nothing."""
import numpy as np
import torch
import torch.nn.functional as F

from codec_ref import RefCodec, snake

U = 2.0 ** -24                                                  # unit roundoff of fp32


def planes_of(x, planes):
    """float64 tensor -> its bf16 planes as float64 tensors: through fp32, hi = bf16(v) round-to-nearest-even, lo = bf16(v - hi)
    with the residual exact in fp32.  planes = 0 is the identity (one 'plane', nothing rounded)."""
    if planes == 0:
        return [x]
    v = x.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    out = [hi.to(torch.float64)]
    if planes == 2:
        out.append((v - hi).to(torch.bfloat16).to(torch.float64))
    return out


def q1(x):
    return planes_of(x, 1)[0]


def q2(x):
    hi, lo = planes_of(x, 2)
    return hi + lo


def products(conv, xs, ws, bias=None):
    """the kernel's products in its order: w_hi x_hi (with the bias, as F.conv1d adds it), then w_hi x_lo and w_lo x_hi; w_lo x_lo is
    dropped.  conv(x, w, bias) is the float64 convolution."""
    y = conv(xs[0], ws[0], bias)
    if len(xs) == 2:
        y = y + conv(xs[1], ws[0], None) + conv(xs[0], ws[1], None)
    return y


class EmuCodec(RefCodec):
    """RefCodec in float64 with every DECODER convolution's folded weight (through fp32, as the host stores it) and every
    convolution input (after Snake) split into `planes` bf16 planes, and exactly the products the kernel forms.  The embedding is
    untouched.  planes = 0 splits nothing and equals RefCodec bit for bit."""

    def __init__(self, cfg, sd, planes):
        super().__init__(cfg, sd, torch.float64)
        self.planes = planes

    def cv(self, fn, x, key, **kw):
        return products(lambda a, w, b: fn(a, w, b, **kw), planes_of(x, self.planes), planes_of(self.w(key), self.planes), self.b(key))

    def decoder(self, z):
        x = self.cv(F.conv1d, z, "decoder.model.0", padding=3)
        for i, s in enumerate(self.cfg.decoder_rates):
            blk = f"decoder.model.{i + 1}.block"
            x = snake(x, self.alpha(f"{blk}.0"))
            x = self.cv(F.conv_transpose1d, x, f"{blk}.1", stride=s, padding=-(-s // 2))
            for u, d in enumerate((1, 3, 9)):
                ru = f"{blk}.{2 + u}.block"
                y = snake(x, self.alpha(f"{ru}.0"))
                y = self.cv(F.conv1d, y, f"{ru}.1", dilation=d, padding=3 * d)
                y = snake(y, self.alpha(f"{ru}.2"))
                y = self.cv(F.conv1d, y, f"{ru}.3")
                x = x + y
        n = len(self.cfg.decoder_rates)
        x = snake(x, self.alpha(f"decoder.model.{n + 1}"))
        x = self.cv(F.conv1d, x, f"decoder.model.{n + 2}", padding=3)
        return torch.tanh(x)


def acc_bound(w, v, planes, conv, n, pre=None, out=None, tanh=False, lolo=2.0 ** -18):
    """Bound on |device - float64| for every output of one layer whose device operands are exactly planes_of(w) and planes_of(v),
    the float64 side being products() over those planes: the emulation of the layer.

    An fp32 sum of n terms t_j in any order is within gamma_(n-1) sum |t_j| of the exact sum, gamma_k = k u / (1 - k u), u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); the products of two bf16 are exact in fp32.  The kernel
    sums its `planes`^2 - (planes - 1)^2 products per (channel, tap) in blocks and adds the blocks, which is one such order with at
    most two more additions per term, so gamma = (n + 2) u with n the number of accumulated products covers it, the derivation
    tests/resample_ref.py uses for its dot products.  `conv(input, weight)` is the layer's float64 convolution without bias, so
    that conv(|v|, |w|) is sum |w_j| |v_j| per output; n = planes-products x C_in x taps.
    planes = 2 adds `lolo` sum |w_j| |v_j| for the dropped w_lo v_lo: 2^-18, the figure the modes were specified with.  Against
    products(), which drops that term too, it is slack.  Against the FULL product of the plane sums, (w_hi + w_lo) (v_hi + v_lo), it
    is no worst case: |lo| <= 2^-8 |value| at the bottom of a binade (bf16 has 8 significant bits), so the dropped term can reach
    2^-16 of that sum, and a caller that compares with the full product passes lolo = 2^-16.
    The epilogue rounds the bias add (u |pre|, pre = sum + bias), the residual add (u |out|) and, with tanh, tanhf: its slope is at
    most 1, so what came in goes out no larger, plus 4 u for the function itself (2 ulp of a result below 1, rounded once more).
    The whole is scaled by 1 + 2^-10 for the second-order terms and for |pre|, |out| being taken from the float64 result."""
    wp, vp = planes_of(w, planes), planes_of(v, planes)
    a = conv(vp[0].abs(), wp[0].abs())
    if planes == 2:
        a = a + conv(vp[1].abs(), wp[0].abs()) + conv(vp[0].abs(), wp[1].abs())
    bound = (n + 2) * U * a
    if planes == 2:
        bound = bound + lolo * conv((vp[0] + vp[1]).abs(), (wp[0] + wp[1]).abs())
    if pre is not None:
        bound = bound + U * pre.abs()
    if out is not None:
        bound = bound + U * out.abs()
    if tanh:
        bound = bound + 4 * U
    return bound * (1 + 2.0 ** -10)


def boundary_distance(y):
    """distance of every float64 value to the nearest rounding boundary of bf16 (a midpoint between two neighbouring bf16 values of
    its binade)"""
    a = y.abs().clamp_min(2.0 ** -120)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    f = a / ulp
    return ((f - torch.floor(f)) - 0.5).abs() * ulp


def settle_margin(x, alpha):
    return 2.0 ** -18 * (x.abs() + 1.0 / alpha)


def settle(x, alpha, g):
    """x fp32-valued float64 [B, C, T], alpha [C]: every element whose float64 Snake value lies within 2^-18 (|x| + 1 / alpha) of a
    rounding boundary of the hi plane is drawn again from N(0, 1) until none is left, so that an fp32 Snake a few ulp off the float64
    one rounds to the same hi.  Asserts that the fp32 torch Snake of the result is within a quarter of that margin of the float64
    one: the reference alone stays inside the condition.  -> (x, fraction re-drawn in the first pass)"""
    al = alpha.reshape(1, -1, 1).to(torch.float64)
    x = x.clone()
    first = None
    for _ in range(64):
        bad = boundary_distance(snake(x, al)) < settle_margin(x, al)
        first = float(bad.double().mean()) if first is None else first
        if not bad.any():
            break
        x[bad] = torch.randn(int(bad.sum()), generator=g, dtype=torch.float32).double()
    assert not (boundary_distance(snake(x, al)) < settle_margin(x, al)).any()
    s32 = snake(x.float(), al.float()).double()
    assert ((s32 - snake(x, al)).abs() <= settle_margin(x, al) / 4).all()
    return x, first


def snr_db(y, ref):
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(10.0 * np.log10((ref ** 2).sum() / max(((y - ref) ** 2).sum(), 1e-300)))
