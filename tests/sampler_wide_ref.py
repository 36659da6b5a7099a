"""float64 numpy restatement of the candidate chain over more than 64 candidates (top_k <= 0,
top_k >= V or top_k > 64 -- the rows the wide kernel picks) and the case table its tests share.

For a row x[0..V) after bias and penalties (sampler_ext_ref.rewrite):

    candidates  the first k tokens in the order value descending, ties to the lower id; k = V when top_k <= 0 or
                top_k >= V, else top_k.  x0 = the first candidate
    e_i = exp(x_i - x0), S = sum_{i<k} e_i, p_i = e_i / S
    top_p < 1   keep through the first i with sum_{j<=i} p_j >= top_p
    min_p > 0   of those, keep through the last i with p_i >= min_p p_0; at least one stays
    w_i = exp(x_i / temp - x0 / temp), u = u01 * sum_kept w_i
    the pick    the first kept i with u < sum_{j<=i} w_j; the last kept candidate when rounding puts u past the end

sampler_ext_ref's 1e-6 mass margin cannot serve here: over 128k candidates the cumulative steps are ~8e-6 and it
would leave out 7 % of the table.  Both implementations carry about 1e-13 of mass, so the margins are 1e-9.
"""
import numpy as np

import sampler_ext_ref as R

MASS_MARGIN = 1e-9   # probability mass: the top-p sum and the draw boundaries
RATIO_MARGIN = 1e-9  # |p_i / (min_p p_0) - 1| for min_p
TOPK_MAX = 64

VOCABS = [1, 2, 3, 63, 64, 65, 66, 2047, 2049, 4097, 32000, 128256]
ROW_COUNTS = (64, 3, 1)
TOP_KS = lambda V: (0, 65, 100, V - 1, -1, V, V + 5, 1000)  # noqa: E731
EVEN = ((1.0, 0.0), (0.95, 0.0), (1.0, 0.02))


def k_eff(s, V: int) -> int:
    k = dict(R.DEFAULTS, **s)["top_k"]
    return V if k <= 0 or k >= V else k


def is_wide(s, V: int) -> bool:
    """The row takes the wide kernel (mx_sample_plan's MX_PICK_WIDE, for the settings of this table)."""
    s = dict(R.DEFAULTS, **s)
    return s["temperature"] > 0 and s["mirostat_mode"] != 2 and k_eff(s, V) > TOPK_MAX


def chain(x, s, u01: float, mu: float = 0.0):
    """As sampler_ext_ref.chain (the same result dict) for a sampled row without tail-free / typical cuts, of any
    number of candidates, under this file's margins; greedy, Mirostat and tail-free / typical rows go to
    sampler_ext_ref.chain itself."""
    s = dict(R.DEFAULTS, **s)
    x = np.asarray(x, dtype=np.float32)
    V = len(x)
    plain = s["temperature"] > 0 and s["mirostat_mode"] != 2 and s["tfs_z"] >= 1 and s["typical_p"] >= 1
    if not plain or k_eff(s, V) <= 1:
        return R.chain(x, s, u01, mu)
    temp = float(np.float32(s["temperature"]))
    margins = []
    res = dict(tok=None, mu_out=mu, margins=margins, kept=None)
    k = k_eff(s, V)
    x64 = x.astype(np.float64)
    order = np.lexsort((np.arange(V), -x64))[:k]  # -0.0 == +0.0: ties to the lower id
    vals = x64[order]
    if vals[0] == -np.inf:
        return res  # no distribution: any token inside the vocabulary
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(vals - vals[0])
    p = e / e.sum()
    keep = k
    top_p, min_p = float(np.float32(s["top_p"])), float(np.float32(s["min_p"]))
    if top_p < 1:
        cum = np.cumsum(p)
        hit = np.flatnonzero(cum >= top_p)
        upto = int(hit[0]) if len(hit) else k - 1
        margins.append((float(np.abs(cum[:upto + 1] - top_p).min()), MASS_MARGIN))
        keep = upto + 1
    if min_p > 0:
        if keep > 1:
            margins.append((float(np.abs(p[1:keep] / (min_p * p[0]) - 1.0).min()), RATIO_MARGIN))
        ok = np.flatnonzero(p[1:keep] >= min_p * p[0])
        keep = int(ok[-1]) + 2 if len(ok) else 1
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(vals[:keep] / temp - vals[0] / temp)
    cum = np.cumsum(w)
    uS = u01 * cum[-1]
    if keep > 1:
        margins.append((float(np.abs(uS - cum[:-1]).min() / cum[-1]), MASS_MARGIN))
    hit = np.flatnonzero(uS < cum)
    res["tok"] = int(order[hit[0]]) if len(hit) else int(order[keep - 1])
    return res


def decided(res) -> bool:
    return all(d >= lim for d, lim in res["margins"])


def make_call(V: int, n: int):
    """sampler_ext_ref.make_call(V, n, salt=2) with the non-Mirostat rows turned to wide settings; the Mirostat
    rows stay, so every call is a mixed batch (and rows whose k comes out <= 64 stay on the per-row chain)."""
    call = R.make_call(V, n, salt=2)
    for i, (s, m) in enumerate(zip(call["settings"], call["miro"])):
        if m:
            continue
        s["tfs_z"] = s["typical_p"] = 1.0
        s["top_k"] = TOP_KS(V)[(i + n) % 8]
        s["top_p"], s["min_p"] = (0.9, 0.05) if i % 2 else EVEN[(i // 2) % 3]
    return call


def reference(call):
    """[(rewritten row f32 [V], chain result)] per row of a call."""
    out = []
    for i, s in enumerate(call["settings"]):
        x = R.rewrite(call["logits"][i, :call["V"]], s, call["windows"][i])
        out.append((x, chain(x, s, R.samp_u01(call["seeds"][i], call["n_drawn"][i]), float(call["mu_in"][i]))))
    return out


_CACHE = {}


def table(V: int):
    """[(call, reference)] for the row counts of one V, computed once per process and shared (left unchanged)."""
    if V not in _CACHE:
        _CACHE[V] = [(c, reference(c)) for c in (make_call(V, n) for n in ROW_COUNTS)]
    return _CACHE[V]
