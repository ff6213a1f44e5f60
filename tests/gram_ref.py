"""References for the Gram matrices (csrc/gram.hip, DESIGN.md "Gram matrices and GPTQ").

kernel_ref: dia_act_gram from a plain [M, K] matrix, the float32 row scale (calib_ref.row_scale_f32) and the gate
(calib_ref.gate): float64 throughout, G += outer(v, v) per counted row, in ascending row order.  Without a scale v is the float32
input widened, the products are exact and the sum takes the device's roundings in the device's order: the result is the device's,
bit for bit.

OracleGram: the same matrices from the float32 oracle.  ``oracle.dia_oracle.dense`` is wrapped as calib_ref.OracleCapture wraps
it, and X^T X of the input rows of every call is summed in float64 under the identity of the weight tensor.  The oracle itself is
not touched.

gptq_case: the three synthetic calibration problems of the GPTQ tests (correlated channels of very unequal power).
"""
import numpy as np


def kernel_ref(x, on, scale=None):
    """(float64 [K, K] Gram matrix of the counted rows of x [M, K] times the float32 row scale, number of counted rows)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    s = np.ones(x.shape[0]) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64)
    K = x.shape[1]
    G = np.zeros((K, K), dtype=np.float64)
    tmp = np.empty((K, K), dtype=np.float64)
    for m in range(x.shape[0]):
        if on[m]:
            v = x[m] * s[m]
            np.multiply(v[:, None], v[None, :], out=tmp)
            G += tmp
    return G, int(np.asarray(on).sum())


class OracleGram:
    """cap = OracleGram(monkeypatch); cap.on = True / False around the oracle calls whose rows count.
    gram[id(weight)] float64 [K, K], rows[id(weight)] int"""

    def __init__(self, monkeypatch, keep=None):
        from oracle import dia_oracle as O
        self.on = False
        self.gram, self.rows = {}, {}
        self.keep = keep                      # ids of the weights to capture (None: all)
        inner = O.dense

        def dense(x, w, n_in=1):
            if self.on and (self.keep is None or id(w) in self.keep):
                k = 1
                for v in w.shape[:n_in]:
                    k *= v
                r = x.reshape(-1, k).double()
                key = id(w)
                self.gram[key] = self.gram.get(key, 0) + (r.t() @ r).numpy()
                self.rows[key] = self.rows.get(key, 0) + r.shape[0]
            return inner(x, w, n_in)

        monkeypatch.setattr(O, "dense", dense)


def oracle_grams(monkeypatch, cfg, sd, texts, rows, names, stop_at=None):
    """The Gram matrices a calibrate="gram" session should report for the kernels ``names``: per utterance decode_step for
    cur = 1 .. rows - 1, counted iff stop_at is None or cur < stop_at[b] — both CFG rows.  Returns ({name: [K, K]}, {name: rows})."""
    from dia_hip.tokens import effective_text
    from oracle import dia_oracle as O
    dm = O.Dims.of(cfg)
    cap = OracleGram(monkeypatch, keep={id(sd[k]) for k in names})
    for b, text in enumerate(texts):
        st = O.prepare(sd, dm, O.text_tokens(effective_text(text), dm), False)
        for cur in range(1, rows[b].shape[0]):
            cap.on = stop_at is None or stop_at[b] is None or cur < stop_at[b]
            O.decode_step(sd, st, rows[b][cur - 1], cur)
    cap.on = False
    return {k: cap.gram[id(sd[k])] for k in names}, {k: cap.rows[id(sd[k])] for k in names}


GPTQ_CASES = [(512, 256, 66), (512, 256, 2048), (1024, 128, 66)]          # (K, N, calibration rows)


def gptq_case(rs, K, N, M):
    """(W float32 [K, N], X float64 [M, K] of float32 values, G = X^T X, Gh of M held-out rows of the same source): inputs mixed from
    K / 4 sources through channels whose power spreads over decades, plus a little independent noise"""
    mix = rs.randn(K, K) * (rs.rand(K) ** 3)[None]
    X = (rs.randn(M, K // 4) @ mix[: K // 4] + 0.1 * rs.randn(M, K)).astype(np.float32).astype(np.float64)
    W = (rs.randn(K, N) * 0.02).astype(np.float32)
    Xh = rs.randn(M, K // 4) @ mix[: K // 4] + 0.1 * rs.randn(M, K)
    return W, X, X.T @ X, Xh.T @ Xh


def output_error(G, delta):
    """tr(delta^T G delta) = ||X delta||_F^2 for G = X^T X: the layer's squared output error on the calibration rows"""
    delta = np.asarray(delta, dtype=np.float64)
    return float(np.einsum("kn,kn->", delta, G @ delta))
