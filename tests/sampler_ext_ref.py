"""float64 numpy restatement of the extended sampler chain and the case table the sampler tests
share.  Written from the chain's specification -- llama-cpp-python 0.3.1's _init_sampler order:

    logit_bias -> penalties -> greedy (temperature <= 0)
                             | temperature -> Mirostat v2 over the whole vocabulary (mirostat_mode == 2)
                             | top_k -> tail-free -> locally typical -> top_p -> min_p -> temperature -> draw

Every decision the chain takes against a threshold is reported with its margin, so a test can leave out the cases
an f32 / f64 implementation may legitimately decide the other way.
"""
import numpy as np

M64 = (1 << 64) - 1
LN2 = float(np.log(2.0))
MASS_MARGIN = 1e-6   # probability mass: draw boundaries and truncation sums
BITS_MARGIN = 1e-3   # Mirostat surprise vs mu, in bits (the f32 log-prob kernels are pinned to 1.5e-4 bits)

# the defaults of engine.sampling() / Engine.submit() (temperature 0: greedy)
DEFAULTS = dict(temperature=0.0, top_k=40, top_p=0.95, min_p=0.05, repeat_penalty=1.0, repeat_last_n=64,
                frequency_penalty=0.0, presence_penalty=0.0, typical_p=1.0, tfs_z=1.0, mirostat_mode=0,
                mirostat_tau=5.0, mirostat_eta=0.1, logit_bias=None)


def samp_u01(seed: int, n: int) -> float:
    """The engine's counter-based uniform draw (kernels.h samp_u01: splitmix64 of seed and draw index)."""
    z = (seed + 0x9E3779B97F4A7C15 * (n + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 11) / 9007199254740992.0


def rewrite(row, s, window):
    """The row as the chain leaves it, in f32: one add per bias entry, then the penalties sampler over the last
    repeat_last_n window tokens (a counted token's logit divided by `repeat` when positive, multiplied when not;
    then count * freq + presence subtracted) -- every operation rounded to f32, in that order."""
    s = dict(DEFAULTS, **s)
    f = np.float32
    out = np.asarray(row, dtype=np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for t, b in (s["logit_bias"] or {}).items():
            out[t] = f(out[t] + f(b))
        repeat, freq, pres = f(s["repeat_penalty"]), f(s["frequency_penalty"]), f(s["presence_penalty"])
        if (repeat != 1 or freq != 0 or pres != 0) and s["repeat_last_n"] != 0:
            last_n = s["repeat_last_n"]
            hist = list(window)[-last_n:] if last_n > 0 else list(window)
            ids, counts = np.unique(np.asarray(hist, np.int64), return_counts=True)
            for t, c in zip(ids, counts):
                v = out[t]
                if repeat != 1:
                    v = f(v * repeat) if v <= 0 else f(v / repeat)
                # count * freq + presence is one fused multiply-add: exact in f64 (a small integer times an f32,
                # plus an f32), rounded to f32 once
                out[t] = f(v - f(np.float64(c) * np.float64(freq) + np.float64(pres)))
    return out


def _softmax(v):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(v - v.max())
        return e / e.sum()


def chain(x, s, u01: float, mu: float):
    """The pick over the rewritten row x (f32 [V]).  Returns dict(tok, mu_out, margins, kept):
    tok None = every candidate is -inf (any token inside the vocabulary is right); margins: list of
    (distance, limit) -- the case is decided only when every distance >= its limit; kept: the Mirostat kept set."""
    s = dict(DEFAULTS, **s)
    x = np.asarray(x, dtype=np.float32)
    V = len(x)
    temp = float(np.float32(s["temperature"]))
    margins = []
    res = dict(tok=None, mu_out=mu, margins=margins, kept=None)
    if temp <= 0:
        res["tok"] = int(np.argmax(x))  # first maximum: ties to the lowest id
        return res
    if s["mirostat_mode"] == 2:
        tau, eta = float(np.float32(s["mirostat_tau"])), float(np.float32(s["mirostat_eta"]))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            y = x.astype(np.float64) / temp
            m = y.max()
            if m == -np.inf:
                res["tok"], res["mu_out"] = None, mu - eta * (0.0 - tau)
                return res
            lp = (y - m) - np.log(np.exp(y - m).sum())
            sur = -lp / LN2
        # the nearest surprise to mu among the tokens whose membership can change the outcome: every token but
        # the (first) argmax -- it has the lowest surprise, so kept alone or as the fallback of an empty set it is
        # the pick with p' = 1 either way, and with others kept it is never the one nearest to mu from below
        fin = np.isfinite(sur)
        fin[int(np.argmax(x))] = False
        if fin.any():
            margins.append((float(np.abs(sur[fin] - mu).min()), BITS_MARGIN))
        kept = sur <= mu
        res["kept"] = kept
        if not kept.any():
            tok, pp = int(np.argmax(x)), 1.0
        else:
            p = np.where(kept, np.exp(lp), 0.0)
            S = p.sum()
            cum = np.cumsum(p)
            ks = np.flatnonzero(kept)
            uS = u01 * S
            hit = ks[uS < cum[ks]]
            tok = int(hit[0]) if len(hit) else int(ks[-1])
            if len(ks) > 1:
                margins.append((float(np.abs(uS - cum[ks[:-1]]).min()), MASS_MARGIN))
            pp = p[tok] / S
        res["tok"], res["mu_out"] = tok, mu - eta * (-np.log2(pp) - tau)
        return res
    # candidates: value descending, ties to the lower id
    k = min(s["top_k"], V) if s["top_k"] > 0 else V
    order = np.lexsort((np.arange(V), -x.astype(np.float64)))[:k]
    vals = x[order].astype(np.float64)
    ids = order
    if k <= 1:
        res["tok"] = int(ids[0])
        return res
    z, tp = float(np.float32(s["tfs_z"])), float(np.float32(s["typical_p"]))
    if vals[0] == -np.inf:
        return res  # nothing but banned tokens
    if z < 1 and k > 2:
        p = _softmax(vals)
        d1 = p[:-1] - p[1:]
        d2 = np.abs(d1[:-1] - d1[1:])
        tot = d2.sum()
        margins.append((abs(tot - 1e-6), 1e-9))
        d2 = d2 / tot if tot > 1e-6 else np.full(k - 2, 1.0 / (k - 2))
        cum = np.cumsum(d2)
        cut = next((i for i in range(1, k - 2) if cum[i] > z), None)
        upto = cut if cut is not None else k - 3
        if upto >= 1:
            margins.append((float(np.abs(cum[1:upto + 1] - z).min()), MASS_MARGIN))
        if cut is not None:
            vals, ids, k = vals[:cut], ids[:cut], cut
    if tp < 1:
        q = _softmax(vals)
        with np.errstate(divide="ignore", invalid="ignore"):
            nl = -np.log(q)
            H = float(np.where(q > 0, q * nl, 0.0).sum())
            sc = np.abs(nl - H)
        o = np.argsort(sc, kind="stable")
        cum = np.cumsum(q[o])
        cut = next((j for j in range(k) if cum[j] > tp), None)
        upto = cut if cut is not None else k - 1
        margins.append((float(np.abs(cum[:upto + 1] - tp).min()), MASS_MARGIN))
        if cut is not None:
            keep = np.sort(o[:cut + 1])  # value order again
            vals, ids, k = vals[keep], ids[keep], len(keep)
    if k <= 1:
        res["tok"] = int(ids[0])
        return res
    p = _softmax(vals)
    keep = k
    top_p, min_p = float(np.float32(s["top_p"])), float(np.float32(s["min_p"]))
    if top_p < 1:
        cum = np.cumsum(p)
        cut = next((i for i in range(k) if cum[i] >= top_p), None)
        upto = cut if cut is not None else k - 1
        margins.append((float(np.abs(cum[:upto + 1] - top_p).min()), MASS_MARGIN))
        if cut is not None:
            keep = cut + 1
    if min_p > 0:
        if keep > 1:
            margins.append((float(np.abs(p[1:keep] - min_p * p[0]).min()), MASS_MARGIN))
        kk = 1
        for i in range(1, keep):
            if p[i] >= min_p * p[0]:
                kk = i + 1
        keep = kk
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(vals[:keep] / temp - vals[0] / temp)
    cum = np.cumsum(w)
    uS = u01 * cum[-1]
    if keep > 1:
        margins.append((float(np.abs(uS - cum[:-1]).min() / cum[-1]), MASS_MARGIN))
    hit = np.flatnonzero(uS < cum)
    res["tok"] = int(ids[hit[0]]) if len(hit) else int(ids[keep - 1])
    return res


def decided(res) -> bool:
    return all(d >= lim for d, lim in res["margins"])


def mu_tol(s, mu_in: float) -> float:
    """|mu_out - reference|: the observed surprise carries at most ~3e-4 bits of f32 error (one log-prob at 1e-4
    plus the kept-mass sum): eta * 1e-3 covers it 3x; the second term is the f32 rounding of mu."""
    return dict(DEFAULTS, **s)["mirostat_eta"] * 1e-3 + 1e-5 * max(1.0, abs(mu_in))


# ---- the case table -------------------------------------------------------------------------------------------
VOCABS = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4097, 32000, 128256]
ROW_COUNTS = [64, 3, 1]
# row kinds, weighted: rows of equal values sit on most thresholds exactly (1/2 of 64 equal masses is exactly
# typical_p = 0.5) and are left out by the margin rule, so they are the rarer kinds
KINDS = ["equal"] + ["onehot"] * 4 + ["twolevel"] * 5 + ["ramp"] * 6 + ["normal"] * 10 + ["wide"] * 9 + ["neginf"] * 5
KIND_STEP = 7  # row g is of kind KINDS[(KIND_STEP * g + g // len(KINDS)) % len(KINDS)]: co-prime with the grid sizes


def _row(kind, V, rng):
    if kind == "equal":
        return np.full(V, rng.normal(), dtype=np.float32)
    if kind == "onehot":
        r = np.full(V, -50.0, dtype=np.float32)
        r[rng.integers(V)] = 50.0
        return r
    if kind == "twolevel":
        r = np.zeros(V, dtype=np.float32)  # one token over a floor: two equal top values would put the tail-free
        r[rng.integers(V)] = 2.5            # cut at exactly z = 0.5 in every such row
        return r
    if kind == "ramp":
        return rng.permutation(np.linspace(-6.0, 6.0, V)).astype(np.float32)
    if kind == "normal":
        return rng.normal(size=V).astype(np.float32)
    if kind == "wide":
        return (8.0 * rng.normal(size=V)).astype(np.float32)
    r = rng.normal(size=V).astype(np.float32)  # neginf: a third of the row banned already
    r[rng.random(V) < 0.33] = -np.inf
    return r


def _candidate_settings():
    out = []
    for typ in (0.2, 0.5, 0.9, 1.0):
        for tfs in (0.5, 0.95, 1.0):
            for top_k in (1, 2, 3, 40, 64):
                for top_p, min_p in ((1.0, 0.0), (0.9, 0.05)):
                    out.append(dict(typical_p=typ, tfs_z=tfs, top_k=top_k, top_p=top_p, min_p=min_p))
    return out


def _miro_settings():
    out = []
    for tau, eta in ((5.0, 0.1), (1.0, 0.5), (0.1, 1.0)):
        for mu_kind in ("start", "zero", "huge"):
            out.append((dict(mirostat_mode=2, mirostat_tau=tau, mirostat_eta=eta),
                        {"start": 2.0 * tau, "zero": 0.0, "huge": 1e3}[mu_kind]))
    return out


CAND, MIRO = _candidate_settings(), _miro_settings()


def make_call(V: int, n: int, salt: int = 0):
    """One probe call: n rows over a vocabulary of V, ldl > V with NaN in the padding.  Row g of the table (a
    running index over every call of this V) takes its row kind, its settings, its bias table and its penalties
    from g, so the calls of one V walk through the whole grid.  Returns dict(logits, V, settings, seeds, n_drawn,
    windows, mu_in, miro [n] bool)."""
    rng = np.random.default_rng(1000003 * V + 7919 * n + salt)
    ldl = V + 1 + (V % 5)
    logits = np.full((n, ldl), np.nan, dtype=np.float32)
    base = {64: 0, 3: 64, 1: 67}.get(n, 0) + 68 * VOCABS.index(V) if V in VOCABS else 0
    settings, seeds, n_drawn, windows, mu_in, miro = [], [], [], [], [], []
    for i in range(n):
        g = base + i
        logits[i, :V] = _row(KINDS[(KIND_STEP * g + g // len(KINDS)) % len(KINDS)], V, rng)
        is_miro = g % 3 == 2
        if is_miro:
            s, mu = MIRO[(g // 3) % len(MIRO)]
            s = dict(s, temperature=(1.0, 0.7)[(g // 27) % 2])
        else:
            s, mu = dict(CAND[(g - g // 3) % len(CAND)], temperature=(0.8, 1.0, 0.9)[g % 3]), 0.0
        win = [int(t) for t in rng.integers(0, V, size=int(rng.integers(1, 40)))]
        if g % 4 == 1:
            s.update(repeat_penalty=1.2, frequency_penalty=0.4, presence_penalty=0.7, repeat_last_n=32)
        bias_kind = g % 5
        if bias_kind == 1:
            s["logit_bias"] = {int(rng.integers(V)): 3.5}
        elif bias_kind == 2:  # a full table, a tenth of it bans
            toks = rng.choice(V, size=min(256, V), replace=False)
            s["logit_bias"] = {int(t): (-np.inf if rng.random() < 0.1 else float(rng.normal() * 4)) for t in toks}
        elif bias_kind == 3:  # on a token the penalties rewrite too
            s["logit_bias"] = {win[-1]: -2.25}
        elif bias_kind == 4 and V > 1:
            s["logit_bias"] = {win[-1]: -np.inf}
        settings.append(s)
        seeds.append(int(rng.integers(1, 2**40)))
        n_drawn.append(g % 64)
        windows.append(win)
        mu_in.append(mu)
        miro.append(is_miro)
    return dict(logits=logits, V=V, settings=settings, seeds=seeds, n_drawn=n_drawn, windows=windows,
                mu_in=np.asarray(mu_in, dtype=np.float32), miro=np.asarray(miro))


def reference(call):
    """[(rewritten row f32 [V], chain result)] per row of a call."""
    out = []
    for i, s in enumerate(call["settings"]):
        x = rewrite(call["logits"][i, :call["V"]], s, call["windows"][i])
        out.append((x, chain(x, s, samp_u01(call["seeds"][i], call["n_drawn"][i]), float(call["mu_in"][i]))))
    return out
