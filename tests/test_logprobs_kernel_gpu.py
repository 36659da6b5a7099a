"""The log-prob kernels (kernels.hip lse_topk_stage1 / logprob_finish_kernel / logprob_gather_kernel) on
crafted rows through mx_logprob_probe -- no model.

Reference: float64 numpy over the same f32 logits, (x - m) - log sum exp(x - m).  Tolerance 1e-4 absolute
on every log-prob: f32 exp / log are good to a few ulp and a fixed-order sum of <= 128256 terms in <= 64
slices carries a relative error of a few tens of ulp on s, ~1e-6 in the log -- 1e-4 leaves > 10x margin
and is far below the 0.016 that one dropped slice of 63 would shift the result by.  Top-k ids are
compared exactly against np.lexsort((ids, -vals)) (value descending, ties -> lower id).

Rows per vocabulary size V (the row bank, reference computed once per V):
  * random rows 4*N(0,1), rounded to multiples of 2^-10 so that the +-1000 shifts below are exact in f32
    (the shifted rows then hold exactly the same distribution, and the rounding makes ties frequent);
  * the same row shifted by +1000 and by -1000 (a naive exp overflows / underflows): results equal the
    unshifted row's within 1e-4;
  * a one-hot row (one entry at 50, the rest at -50): the peak's |lp| <= 1e-4, the others ~ -100;
  * an all-equal row: every log-prob is -ln V and the top ids are 0..k-1;
  * identical rows at different row indices and different n: bitwise-equal outputs.
V in {1, 63, 512, 4097, 32000, 128256}: one slice, a ragged slice boundary, 63 uneven slices; n in
{1, 3, 64}; k in {0, 1, 5, 64} clipped to V; targets include ids 0 and V-1; one case has ldl > V.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
VS = [1, 63, 512, 4097, 32000, 128256]
KS = [0, 1, 5, 64]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def ref_logprobs(x):
    x = x.astype(np.float64)
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum())


@functools.lru_cache(maxsize=None)
def ref_top64(V, kd):
    x = bank(V)[kd][0]
    return np.lexsort((np.arange(V), -x.astype(np.float64)))[:64]


@functools.lru_cache(maxsize=None)
def bank(V):
    """[(row f32 [V], target id, float64 reference log-probs)] -- built and referenced once per V."""
    rng = np.random.default_rng(1000 + V)
    r0 = (np.round(4.0 * rng.standard_normal(V) * 1024.0) / 1024.0).astype(np.float32)
    r1 = (4.0 * rng.standard_normal(V)).astype(np.float32)
    peak = V // 3
    hot = np.full(V, -50.0, np.float32)
    hot[peak] = 50.0
    flat = np.full(V, 0.5, np.float32)
    up, down = r0 + np.float32(1000.0), r0 - np.float32(1000.0)
    assert np.array_equal(up - np.float32(1000.0), r0) and np.array_equal(down + np.float32(1000.0), r0)
    rows = [(r0, 0), (up, 0), (down, 0), (hot, peak), (hot, V - 1), (flat, V - 1), (r1, V - 1), (r1, V // 2)]
    out = []
    for x, t in rows:
        x.setflags(write=False)
        out.append((x, t, ref_logprobs(x)))
    return out


def run(mx, V, kinds, k, ldl=None):
    b = bank(V)
    lg = np.zeros((len(kinds), ldl or V), np.float32)
    if ldl:
        lg[:] = 1e30  # columns past V must never be read as logits
    for i, kd in enumerate(kinds):
        lg[i, :V] = b[kd][0]
    return mx.logprob_probe(lg, [b[kd][1] for kd in kinds], k, V=V)


def check_rows(V, kinds, k, got):
    b = bank(V)
    tgt, top, idx = got
    ke = min(k, V)
    assert tgt.shape == (len(kinds),) and top.shape == idx.shape == (len(kinds), ke)
    for i, kd in enumerate(kinds):
        x, t, ref = b[kd]
        assert abs(tgt[i] - ref[t]) <= TOL, f"V={V} kind {kd} row {i}: target lp {tgt[i]} vs {ref[t]}"
        want = ref_top64(V, kd)[:ke]
        assert idx[i].tolist() == want.tolist(), f"V={V} kind {kd} row {i} k={k}: top ids"
        err = np.abs(top[i] - ref[want]).max() if ke else 0.0
        assert err <= TOL, f"V={V} kind {kd} row {i} k={k}: top lp max err {err}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", VS)
def test_logprobs_vs_float64(mx, V, k):
    nk = len(bank(V))
    ke = min(k, V)
    single = [run(mx, V, [kd], k) for kd in range(nk)]                 # n = 1
    for kd in range(nk):
        check_rows(V, [kd], k, single[kd])
    trips = [[0, 1, 2], [3, 5, 6], [4, 7, 0]]                          # n = 3
    got3 = [run(mx, V, kinds, k) for kinds in trips]
    for kinds, g in zip(trips, got3):
        check_rows(V, kinds, k, g)
    kinds64 = [(5 * i + 3) % nk for i in range(64)]                    # n = 64
    got64 = run(mx, V, kinds64, k)
    check_rows(V, kinds64, k, got64)

    # the same row at any index and any n: bitwise-equal outputs
    def bits(g, i):
        return g[0][i].tobytes(), g[1][i].tobytes(), g[2][i].tobytes()

    for kinds, g in list(zip(trips, got3)) + [(kinds64, got64)]:
        for i, kd in enumerate(kinds):
            assert bits(g, i) == bits(single[kd], 0), f"V={V} k={k}: kind {kd} at row {i} of {len(kinds)} differs"

    # shifted rows equal the unshifted one
    for sh in (1, 2):
        assert abs(single[sh][0][0] - single[0][0][0]) <= TOL
        assert single[sh][2][0].tolist() == single[0][2][0].tolist()
        if ke:
            assert np.abs(single[sh][1][0] - single[0][1][0]).max() <= TOL
    # one-hot: the peak, and everything else ~ -100
    assert abs(single[3][0][0]) <= TOL
    if V - 1 != V // 3:
        assert abs(single[4][0][0] + 100.0) <= TOL
    if ke >= 2:
        assert np.abs(single[3][1][0][1:] + 100.0).max() <= TOL and abs(single[3][1][0][0]) <= TOL
    # all-equal
    assert abs(single[5][0][0] + np.log(V)) <= TOL
    assert single[5][2][0].tolist() == list(range(ke))
    if ke:
        assert np.abs(single[5][1][0] + np.log(V)).max() <= TOL


@pytest.mark.parametrize("k", [0, 5, 64])
def test_row_stride_wider_than_vocab(mx, k):
    V, kinds = 4097, [0, 6, 3]
    got = run(mx, V, kinds, k, ldl=V + 7)
    check_rows(V, kinds, k, got)
    tight = run(mx, V, kinds, k)
    for a, b in zip(got, tight):
        assert a.tobytes() == b.tobytes()


def test_bad_arguments_are_refused(mx):
    lg = np.zeros((2, 16), np.float32)
    for tg, k in (([0, 16], 1), ([0, -1], 1), ([0, 1], 65), ([0, 1], -1)):
        with pytest.raises(mx.MxError):
            mx.logprob_probe(lg, tg, k)
