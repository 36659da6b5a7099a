"""The embedding tail alone (mx_pool_probe: launch_embd_norm / launch_embd_mean / launch_embd_l2 through the
engine's own launch sequence) against float64 numpy, on rows no model produces.

Shapes: widths 64 and 320 (the generic kernel at its smallest and at a non-power-of-two), 4096 and 8192 (the two
1024-thread layouts); twelve sequences of 1, 2, 15, 16, 17 and 33 rows packed into one call; chunk_rows 0, 16 and
48, so sequences start, end and straddle chunk boundaries; every pooling, with and without normalize.  x ~ N(0, 1)
times a per-row scale in [1e-3, 1e3], w in [0.5, 1.5].

Tolerance (derived, not measured).  With y the float64 rows (x * 1/sqrt(mean(x^2) + eps)) * w: the device forms
the sum of squares in double from f32-rounded squares and f32 tile partials (relative error <= 2 * 2^-24, so
<= 2^-24 on the scale after the square root), rounds mean + eps, the square root, the reciprocal and the two
products once each (<= 2^-25 each): a y element is within 4 * 2^-24 of its reference, relatively.  MEAN adds T - 1
times in f32, each rounding <= 2^-25 of a partial sum that is at most the sum of |y_t[c]| = T * A[c], A[c] = mean_t
|y_t[c]|, then divides by T (one rounding): after the division the T - 1 additions contribute at most
(T - 1) * 2^-25 * A[c].  All of it lies inside (T + 16) * 2^-24 * A[c], the bound asserted; for NONE / CLS / LAST
the chain has no additions: T = 1 and A[c] = |ref[c]|.  With normalize the device divides by its own f32 norm
(canonical double sum, one sqrt, one cast, one division: a few 2^-24 relative), so the bound is the unnormalised one
divided by the reference's unnormalised norm plus 16 * 2^-24 * |ref|.

Bitwise: a sequence's output is the same for every chunk_rows, at any row offset and with any neighbours, and
LAST / CLS equal the matching NONE rows.  An all-zero sequence with normalize gives zeros (no NaN); the 64 guard
rows come back as 0xFF; bad arguments are refused with nothing launched.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))
U = 2.0 ** -24
LENS = [1, 2, 15, 16, 17, 33, 17, 1, 16, 33, 2, 15]  # 168 rows: more than one chunk at 16 and 48
PERM = [5, 0, 9, 3, 11, 2, 7, 4, 1, 10, 6, 8]        # the same sequences in another order (other offsets)
WIDTHS = [64, 320, 4096, 8192]
CHUNKS = [0, 16, 48]
NONE, MEAN, CLS, LAST = 0, 1, 2, 3


def _begins(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _y64(x, w):
    x = x.astype(np.float64)
    return x * (1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + EPS)) * w.astype(np.float64)


def _reference(y, begins, pooling):
    """(ref [vectors][n], bound numerator A * (T + 16) [vectors][n]) before normalisation."""
    if pooling == NONE:
        return y, 17 * np.abs(y)
    ref, bnd = [], []
    for a, b in zip(begins[:-1], begins[1:]):
        if pooling == MEAN:
            ref.append(y[a:b].mean(axis=0))
            bnd.append((b - a + 16) * np.abs(y[a:b]).mean(axis=0))
        else:
            r = y[a] if pooling == CLS else y[b - 1]
            ref.append(r)
            bnd.append(17 * np.abs(r))
    return np.array(ref), np.array(bnd)


@pytest.fixture(scope="module")
def data():
    """Per width: the sequences' rows (list of [len][n] f32), w, and their float64 normed rows -- made once."""
    out = {}
    for n in WIDTHS:
        rng = np.random.default_rng(1000 + n)
        seqs = [(rng.standard_normal((T, n)) * 10.0 ** rng.uniform(-3, 3, (T, 1))).astype(np.float32) for T in LENS]
        w = rng.uniform(0.5, 1.5, n).astype(np.float32)
        out[n] = (seqs, w, [_y64(s, w) for s in seqs])
    return out


def _run(E, seqs, w, order, pooling, normalize, chunk):
    x = np.concatenate([seqs[i] for i in order])
    begins = _begins([len(seqs[i]) for i in order])
    got, guard = E.pool_probe(x, w, begins, pooling, normalize=normalize, chunk_rows=chunk, eps=EPS)
    assert (guard == 0xFFFFFFFF).all(), "guard rows were written"
    return got, begins


@pytest.mark.parametrize("pooling", [NONE, MEAN, CLS, LAST])
@pytest.mark.parametrize("n", WIDTHS)
def test_against_float64_and_bitwise_across_chunks(data, n, pooling):
    from llama_p2p_amd import engine as E

    seqs, w, ys = data[n]
    order = list(range(len(LENS)))
    y = np.concatenate(ys)
    worst = 0.0
    for normalize in (False, True):
        first = None
        for chunk in CHUNKS:
            got, begins = _run(E, seqs, w, order, pooling, normalize, chunk)
            assert got.shape == ((len(y) if pooling == NONE else len(LENS)), n)
            assert np.isfinite(got).all()
            if first is None:
                first = got
                ref, bnd = _reference(y, begins, pooling)
                tol = bnd * U
                if normalize:
                    nrm = np.linalg.norm(ref, axis=1, keepdims=True)
                    ref = ref / nrm
                    tol = tol / nrm + 16 * U * np.abs(ref)
                err = np.abs(got.astype(np.float64) - ref)
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
                bad = np.argwhere(err > tol)
                assert bad.size == 0, (f"n={n} pooling={pooling} normalize={normalize}: {len(bad)} elements outside "
                                       f"the bound, first {bad[0]}, worst err/tol {worst:.3g}")
                if normalize:
                    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 8 * U
            else:  # the carry between chunks is exact: the cut changes no bit
                assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), \
                    f"n={n} pooling={pooling} normalize={normalize}: chunk_rows={chunk} differs from one chunk"
    print({"n": n, "pooling": pooling, "worst_err_over_tol": round(worst, 4)})


@pytest.mark.parametrize("n", WIDTHS)
def test_bitwise_at_any_offset_and_cls_last_are_none_rows(data, n):
    from llama_p2p_amd import engine as E

    seqs, w, _ = data[n]
    ident = list(range(len(LENS)))
    for normalize in (False, True):
        res = {}
        for pooling in (NONE, MEAN, CLS, LAST):
            a, ba = _run(E, seqs, w, ident, pooling, normalize, 48)
            b, bb = _run(E, seqs, w, PERM, pooling, normalize, 16)
            res[pooling] = (a, ba)
            for k, q in enumerate(PERM):  # sequence q sits at position k of the permuted call
                if pooling == NONE:
                    va, vb = a[ba[q]:ba[q + 1]], b[bb[k]:bb[k + 1]]
                else:
                    va, vb = a[q], b[k]
                assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)), \
                    f"n={n} pooling={pooling} normalize={normalize}: sequence {q} depends on its place in the call"
        none, begins = res[NONE]
        assert np.array_equal(res[CLS][0].view(np.uint32), none[begins[:-1]].view(np.uint32))
        assert np.array_equal(res[LAST][0].view(np.uint32), none[begins[1:] - 1].view(np.uint32))
        # a one-row sequence: its mean is the row itself (no addition, x / 1)
        for q, T in enumerate(LENS):
            if T == 1:
                assert np.array_equal(res[MEAN][0][q].view(np.uint32), none[begins[q]].view(np.uint32))


@pytest.mark.parametrize("n", [64, 4096])
def test_zero_sequence_normalizes_to_zeros(n):
    from llama_p2p_amd import engine as E

    rng = np.random.default_rng(7)
    lens = [3, 17, 2]
    x = rng.standard_normal((sum(lens), n)).astype(np.float32)
    x[3:20] = 0.0  # the middle sequence, across a chunk boundary at 16
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    begins = _begins(lens)
    for pooling in (NONE, MEAN, CLS, LAST):
        got, guard = E.pool_probe(x, w, begins, pooling, normalize=True, chunk_rows=16, eps=EPS)
        assert (guard == 0xFFFFFFFF).all()
        assert not np.isnan(got).any()
        mid = got[3:20] if pooling == NONE else got[1]
        assert (mid == 0).all()
        rest = np.concatenate([got[:3], got[20:]]) if pooling == NONE else got[[0, 2]]
        assert np.abs(np.linalg.norm(rest.astype(np.float64), axis=1) - 1).max() < 8 * U


def test_refusals_launch_nothing():
    from llama_p2p_amd import engine as E

    rng = np.random.default_rng(3)

    def refused(rows, n, begins, chunk=0, pooling=MEAN):
        x = rng.standard_normal((rows, n)).astype(np.float32)
        w = np.ones(n, np.float32)
        out = np.full((max(rows, len(begins)) + 64 + 8, max(n, 1)), 123.0, np.float32)
        with pytest.raises(E.MxError) as ei:
            E.pool_probe(x, w, begins, pooling, chunk_rows=chunk, out=out)
        assert ei.value.code == E.MX_ERR_ARG
        assert (out == 123.0).all(), "a refused call wrote its output"

    refused(0, 64, [0])                      # no rows
    refused(4, 96, [0, 4])                   # n % 64 != 0
    refused(1, 16448, [0, 1])                # n > 16384
    refused(10, 64, [0, 5, 5, 10])           # seq_begin does not increase
    refused(10, 64, [0, 7, 5, 10])           # ... decreases
    refused(10, 64, [0, 5])                  # does not cover the rows
    refused(10, 64, [1, 10])                 # does not start at 0
    refused(10, 64, [0, 12])                 # ends past the rows
    refused(32, 64, [0, 32], chunk=8)        # chunk_rows % 16 != 0
    refused(32, 64, [0, 32], chunk=-16)
    refused(32, 64, [0, 32], pooling=4)      # LLAMA_POOLING_TYPE_RANK
    refused(32, 64, [0, 32], pooling=-1)
    got, guard = E.pool_probe(rng.standard_normal((32, 64)).astype(np.float32), np.ones(64, np.float32), [0, 32],
                              MEAN, chunk_rows=16)
    assert np.isfinite(got).all() and (guard == 0xFFFFFFFF).all()
