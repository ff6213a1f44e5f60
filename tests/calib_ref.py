"""References for the activation statistics (csrc/calib.hip, DESIGN.md "Activation statistics").

kernel_ref: dia_act_stats from a plain [M, K] matrix, the strip partial sums and the gate.  The row scale is the header's
expression restated in float32, operation by operation; everything behind it (the product, the squares, the sums) is float64.

OracleCapture: the same statistics from the float32 oracle.  ``oracle.dia_oracle.dense`` is wrapped (``swiglu_mlp`` calls it through
the module, so its two contractions are seen as well) and the squared input rows of every call are summed in float64 under the
identity of the weight tensor the call was handed, while ``encoder_forward``, ``cross_kv`` and ``decode_step`` run teacher-forced.
The oracle itself is not touched.
"""
import numpy as np
import torch


def row_scale_f32(ssq, n, inv_d, eps, M):
    """float32 [M]: q = 0; q += ssq[i][m] for i ascending; 1.0f / sqrtf(q * inv_d + eps) — every operation rounded to float32"""
    q = np.zeros(M, dtype=np.float32)
    for i in range(n):
        q = (q + ssq[i, :M].astype(np.float32)).astype(np.float32)
    t = (q * np.float32(inv_d)).astype(np.float32)
    t = (t + np.float32(eps)).astype(np.float32)
    return (np.float32(1.0) / np.sqrt(t, dtype=np.float32)).astype(np.float32)


def gate(M, row_mask=None, cur=None, first=None, done=None, T=0):
    """bool [M]: which rows count — row_mask and, with cur, the gate of dia_score on utterance m // 2"""
    on = np.ones(M, dtype=bool) if row_mask is None else np.asarray(row_mask[:M]) != 0
    if cur is not None:
        for m in range(M):
            b = m // 2
            f = 1 if first is None else int(first[b])
            d = False if done is None else bool(done[b])
            on[m] &= (f <= int(cur[b]) < T) and int(cur[b]) >= 0 and not d
    return on


def kernel_ref(x, on, scale=None):
    """(float64 [K] sums of squares of the counted rows of x [M, K] times the float32 row scale, number of counted rows)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    s = np.ones(x.shape[0]) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64)
    v = x * s[:, None]
    return (v[on] ** 2).sum(axis=0), int(on.sum())


class OracleCapture:
    """with OracleCapture(monkeypatch) as cap: ... cap.on = True / False around the oracle calls whose rows count.
    sums[id(weight)] float64 [K], rows[id(weight)] int"""

    def __init__(self, monkeypatch):
        from oracle import dia_oracle as O
        self.on = False
        self.sums, self.rows = {}, {}
        inner = O.dense

        def dense(x, w, n_in=1):
            if self.on:
                k = 1
                for v in w.shape[:n_in]:
                    k *= v
                r = x.reshape(-1, k).double()
                key = id(w)
                self.sums[key] = self.sums.get(key, 0) + (r * r).sum(dim=0).numpy()
                self.rows[key] = self.rows.get(key, 0) + r.shape[0]
            return inner(x, w, n_in)

        monkeypatch.setattr(O, "dense", dense)

    def by_name(self, sd, names):
        """({name: sums}, {name: rows}) for the kernels of ``names``, looked up by the identity of sd[name]"""
        return {k: self.sums[id(sd[k])] for k in names}, {k: self.rows[id(sd[k])] for k in names}


def oracle_stats(monkeypatch, cfg, sd, texts, rows, first, stop_at=None):
    """The statistics a calibrating session should report for these utterances: per utterance the lean encoder pass and the
    cross-K/V projection (every text row counts), then decode_step for cur = 1 .. rows - 1, counted iff cur >= first[b] and
    (stop_at is None or cur < stop_at[b]) — both CFG rows.  Returns (sums, counts) by kernel name."""
    from dia_hip.pruning import prunable_names
    from dia_hip.tokens import effective_text
    from oracle import dia_oracle as O
    dm = O.Dims.of(cfg)
    cap = OracleCapture(monkeypatch)
    for b, text in enumerate(texts):
        cap.on = True
        st = O.prepare(sd, dm, O.text_tokens(effective_text(text), dm), False)
        for cur in range(1, rows[b].shape[0]):
            cap.on = cur >= first[b] and (stop_at is None or stop_at[b] is None or cur < stop_at[b])
            O.decode_step(sd, st, rows[b][cur - 1], cur)
    cap.on = False
    return cap.by_name(sd, prunable_names(cfg))
