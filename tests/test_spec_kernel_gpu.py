"""The two kernels of prompt-lookup speculative decoding alone, on inputs no model produces, compared exactly
with numpy (mx_draft_probe / mx_accept_probe run the production launchers without an engine).

  * spec_draft_kernel vs LlamaPromptLookupDecoding.__call__ (the host restatement): sequences over a 4-symbol
    alphabet (many matches, so the lowest index matters), lengths around the 64-lane wave and the 256-thread
    work-group and one of several passes per thread; tokens, n_draft, positions and slots of every row;
  * spec_accept_kernel vs a numpy walk over the rows' argmax (ties -> lowest id, as oracle.argmax_lowest):
    every accepted-prefix length, n_draft = 0, a right token in a padded row, equal maxima in different
    argmax chunks; every output, and 0xFF bytes wherever nothing was to be written.

A speculating forward has R (1 + D) <= 16 rows, so of R in {1, 3} x D in {1, 4, 10, 15} three requests exist
only with D <= 4; the probes refuse the rest (checked).
"""
import numpy as np
import pytest

from llama_p2p_amd.speculative import LlamaPromptLookupDecoding

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 257, 2048]


@pytest.fixture(scope="module")
def mx():
    from llama_p2p_amd import engine

    engine.lib()
    return engine


def check_draft(mx, seqs, D, NG, pos0, slot0):
    ids, pos, slot, nd = mx.draft_probe(seqs, D, NG, pos0=pos0, slot0=slot0)
    look = LlamaPromptLookupDecoding(max_ngram_size=NG, num_pred_tokens=D)
    for r, q in enumerate(seqs):
        ref = look(np.asarray(q, dtype=np.intc)).tolist()
        what = f"len {len(q)} D {D} NG {NG} request {r}"
        assert nd[r] == len(ref), what
        pad = ref[-1] if ref else q[-1]  # rows past n_draft repeat the last valid token
        assert ids[r, 1:].tolist() == ref + [pad] * (D - len(ref)), what
        assert ids[r, 0] == -1, what  # row 0's id is the accept kernel's to write
        assert pos[r].tolist() == [pos0[r] + j for j in range(1 + D)], what
        assert slot[r].tolist() == [slot0[r]] * (1 + D), what


@pytest.mark.parametrize("D", [1, 4, 10, 15])
@pytest.mark.parametrize("NG", [1, 2, 3])
def test_draft_kernel_one_request(mx, D, NG):
    rng = np.random.default_rng(1000 + 16 * NG + D)
    for n in LENGTHS:
        q = rng.integers(0, 4, n).tolist()
        check_draft(mx, [q], D, NG, pos0=[n - 1], slot0=[5])


@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("NG", [1, 2, 3])
def test_draft_kernel_three_requests(mx, D, NG):
    # R = 3 needs 3 (1 + D) <= 16; sequences of different lengths share the call
    rng = np.random.default_rng(2000 + 16 * NG + D)
    for lens in ([1, 2, 3], [63, 64, 65], [257, 2048, 2], [2048, 65, 257]):
        seqs = [rng.integers(0, 4, n).tolist() for n in lens]
        check_draft(mx, seqs, D, NG, pos0=[n + 6 for n in lens], slot0=[2, 0, 7])


def test_draft_kernel_crafted(mx):
    # no match at all (distinct tokens), the match only at size 1, the only full match being the key itself,
    # a continuation shorter than D, a late match far beyond the first pass of the 256 threads
    far = list(range(100, 1900)) + [7, 8, 9, 50, 51] + list(range(2000, 2100)) + [7, 8, 9]
    for q, D, NG in [(list(range(300)), 4, 3), ([5, 7, 8, 9, 7], 3, 2), ([7, 9, 8, 7], 4, 2), ([1, 2, 3, 1, 2], 10, 2),
                     (far, 4, 3), ([4, 4], 5, 2), ([6, 6, 6], 4, 3)]:
        check_draft(mx, [q], D, NG, pos0=[len(q) - 1], slot0=[0])


def test_draft_probe_refuses_bad_arguments(mx):
    for seqs, D, NG, kw in [([[1, 2]] * 3, 10, 2, {}),          # 3 x 11 rows > 16
                            ([[1, 2]], 16, 2, {}), ([[1, 2]], 0, 2, {}), ([[1, 2]], 4, 0, {}),
                            ([[1, 2], []], 4, 2, {}),            # an empty sequence
                            ([[1, 2]], 4, 2, {"pos0": [-1]}), ([[1, 2]], 4, 2, {"slot0": [-1]}),
                            ([[1, 2]] * 9, 1, 1, {})]:
        with pytest.raises(mx.MxError) as ei:
            mx.draft_probe(seqs, D, NG, **kw)
        assert ei.value.code == mx.MX_ERR_ARG


# ------------------------------------------------------------------------------------------------ accept
def argmax_lowest(row):
    return int(np.flatnonzero(row == row.max())[0])


def accept_ref(logits, draft, n_draft, pos0):
    R, D1, _ = logits.shape
    out = {"a": [], "emitted": np.full((R, D1), -1, np.int32), "next_id": [], "new_pos": [], "counts": []}
    for r in range(R):
        am = [argmax_lowest(logits[r, j]) for j in range(D1)]
        a = 0
        while a < n_draft[r] and am[a] == draft[r][a]:
            a += 1
        out["a"].append(a)
        out["emitted"][r, :a + 1] = am[:a + 1]
        out["next_id"].append(am[a])
        out["new_pos"].append(pos0[r] + a + 1)
        out["counts"].append([1, n_draft[r], a])
    return out


def check_accept(mx, logits, draft, n_draft, pos0, what):
    got = mx.accept_probe(logits, draft, n_draft, pos0)
    ref = accept_ref(logits, draft, n_draft, pos0)
    assert got["a"].tolist() == ref["a"], what
    assert np.array_equal(got["emitted"], ref["emitted"]), what  # -1 = the 0xFF pre-fill past a + 1 tokens
    assert got["next_id"].tolist() == ref["next_id"], what
    assert got["new_pos"].tolist() == ref["new_pos"], what
    assert got["counts"].tolist() == ref["counts"], what
    return ref["a"]


def rows_with_argmax(rng, R, D, V, targets):
    """f32 rows [R][1 + D][V] of noise in [-1, 1) whose argmax is targets[r][j] (a 4.0 there)."""
    lg = rng.uniform(-1, 1, (R, 1 + D, V)).astype(np.float32)
    for r in range(R):
        for j in range(1 + D):
            lg[r, j, targets[r][j]] = 4.0
    return lg


@pytest.mark.parametrize("V", [512, 32000, 128256])
@pytest.mark.parametrize("R,D", [(1, 1), (1, 10), (1, 15), (3, 1)])
def test_accept_kernel_every_prefix_length(mx, V, R, D):
    rng = np.random.default_rng(V + 100 * R + D)
    # request r of case `wrong_at`: drafts right up to wrong_at + r (mod D + 1), then wrong; D = all right
    for wrong_at in range(D + 1):
        tg = rng.integers(0, V, (R, 1 + D))
        draft = tg[:, :D].copy()  # draft j is verified by row j's argmax
        want = []
        for r in range(R):
            w = (wrong_at + r) % (D + 1)
            if w < D:
                draft[r, w] = (draft[r, w] + 1 + rng.integers(0, V - 1)) % V
            want.append(w)
        a = check_accept(mx, rows_with_argmax(rng, R, D, V, tg), draft, [D] * R, [7 + 3 * r for r in range(R)],
                         f"V {V} R {R} D {D} wrong at {wrong_at}")
        assert a == want


@pytest.mark.parametrize("V", [512, 128256])
@pytest.mark.parametrize("R,D", [(1, 10), (3, 4), (1, 15)])
def test_accept_kernel_padded_rows_are_never_accepted(mx, V, R, D):
    rng = np.random.default_rng(7 * V + R + D)
    for nd in sorted({0, 1, D // 2, D - 1}):
        # every draft equals its row's argmax -- also in the padded rows past n_draft, which must not count
        tg = rng.integers(0, V, (R, 1 + D))
        a = check_accept(mx, rows_with_argmax(rng, R, D, V, tg), tg[:, :D].copy(), [nd] * R, [0] * R,
                         f"V {V} R {R} D {D} n_draft {nd}")
        assert a == [nd] * R


@pytest.mark.parametrize("V", [512, 32000, 128256])
def test_accept_kernel_ties_take_the_lowest_id(mx, V):
    # equal maxima in different argmax chunks (64 chunks of ceil(V / 64) ids) and inside one chunk
    R, D = 1, 4
    rng = np.random.default_rng(V)
    per = -(-V // 64)
    lg = rng.uniform(-1, 1, (R, 1 + D, V)).astype(np.float32)
    ties = [(3, per + 1, V - 1), (per * 5 + 2, per * 40), (V - 2, V - 1), (per - 1, per), (0, V - 1)]
    for j, ids in enumerate(ties):
        lg[0, j, list(ids)] = 2.5
    low = [min(t) for t in ties]
    # drafts: the lowest tied id (right), except row 2 where the draft is the higher tied id (wrong)
    draft = np.array([[low[0], low[1], ties[2][1], low[3]]])
    a = check_accept(mx, lg, draft, [4], [11], f"V {V} ties")
    assert a == [2]
    draft[0, 2] = low[2]
    assert check_accept(mx, lg, draft, [4], [11], f"V {V} ties, all right") == [4]


def test_accept_probe_refuses_bad_arguments(mx):
    lg = np.zeros((1, 5, 64), np.float32)
    for draft, nd, pos0 in [([[0, 1, 2, 64]], [4], [0]), ([[0, 1, 2, -1]], [4], [0]), ([[0, 1, 2, 3]], [5], [0]),
                            ([[0, 1, 2, 3]], [-1], [0]), ([[0, 1, 2, 3]], [4], [-1])]:
        with pytest.raises(mx.MxError) as ei:
            mx.accept_probe(lg, draft, nd, pos0)
        assert ei.value.code == mx.MX_ERR_ARG
    with pytest.raises(mx.MxError):
        mx.accept_probe(np.zeros((3, 11, 64), np.float32), np.zeros((3, 10), np.int32), [0] * 3, [0] * 3)
