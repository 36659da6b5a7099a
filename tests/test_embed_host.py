"""Llama.embed / create_embedding / pooling_type on the CPU, over a stand-in engine with Engine's embedding
surface (embed(prompts, pooling=, normalize=) and supports_embeddings): the llama-cpp-python 0.3.1 contract as
llama.py's docstring pins it -- str vs list shapes, per-token lists with LLAMA_POOLING_TYPE_NONE, return_count,
truncation to n_batch and the ValueError without it, the RuntimeError without embedding=True, the
create_embedding dict key by key, NotImplementedError on a front without supports_embeddings (the pipeline
server's), the refused pooling_type values, and that normalize reaches the engine and is not applied again.
"""
import numpy as np
import pytest

from llama_p2p_amd import engine as E
from llama_p2p_amd import llama as L
from llama_p2p_amd.llama import Llama

MODEL = "synthetic:test-tiny:seed=0"
N_EMBD = 8


class CannedEngine:
    """Row t of prompt p is [100 p + t + c / 16 for c < N_EMBD] (never unit length); pooled calls return the
    pooling's row of it (MEAN: the mean).  With normalize every value is negated instead of scaled, so a host that
    normalised again -- or a lost flag -- shows."""
    supports_embeddings = True

    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd, self.calls = n_vocab, N_EMBD, []

    def embed(self, prompts, pooling=E.POOL_NONE, normalize=False):
        self.calls.append({"prompts": [list(p) for p in prompts], "pooling": pooling, "normalize": normalize})
        out = []
        for p, ids in enumerate(prompts):
            rows = np.array([[100 * p + t + c / 16 for c in range(N_EMBD)] for t in range(len(ids))], np.float32)
            if pooling == E.POOL_MEAN:
                rows = rows.mean(axis=0, keepdims=True, dtype=np.float32)
            elif pooling == E.POOL_CLS:
                rows = rows[:1]
            elif pooling == E.POOL_LAST:
                rows = rows[-1:]
            out.append(-rows if normalize else rows)
        return out


class NoEmbedEngine:
    def __init__(self, n_vocab=512):
        self.n_vocab, self.n_embd = n_vocab, N_EMBD


def make(embedding=True, eng=None, **kw):
    eng = eng or CannedEngine()
    return Llama.from_engine(MODEL, eng, n_ctx=64, embedding=embedding, **kw), eng


def row(p, t):
    return [float(np.float32(100 * p + t + c / 16)) for c in range(N_EMBD)]


def test_pooling_constants_and_default():
    assert (L.LLAMA_POOLING_TYPE_UNSPECIFIED, L.LLAMA_POOLING_TYPE_NONE, L.LLAMA_POOLING_TYPE_MEAN,
            L.LLAMA_POOLING_TYPE_CLS, L.LLAMA_POOLING_TYPE_LAST) == (-1, 0, 1, 2, 3)
    assert (E.POOL_NONE, E.POOL_MEAN, E.POOL_CLS, E.POOL_LAST) == (0, 1, 2, 3)
    llm, _ = make()
    assert llm.pooling_type() == L.LLAMA_POOLING_TYPE_NONE  # UNSPECIFIED, no llama.pooling_type in the model
    llm, _ = make(pooling_type=L.LLAMA_POOLING_TYPE_LAST)
    assert llm.pooling_type() == L.LLAMA_POOLING_TYPE_LAST


def test_str_and_list_shapes_without_pooling():
    llm, eng = make()
    n = len(llm.tokenize(b"hello world"))
    one = llm.embed("hello world")
    assert isinstance(one, list) and len(one) == n and all(len(r) == N_EMBD for r in one)
    assert one == [row(0, t) for t in range(n)]
    assert all(isinstance(v, float) for r in one for v in r)
    many = llm.embed(["hello world", "a"])
    assert len(many) == 2 and many[0] == one
    assert many[1] == [row(1, t) for t in range(len(llm.tokenize(b"a")))]
    assert llm.embed(["hello world"]) == [one]  # a list of one stays a list
    # tokenised with BOS, every input in ONE engine call
    assert eng.calls[1]["prompts"] == [llm.tokenize(b"hello world"), llm.tokenize(b"a")]
    assert eng.calls[1]["prompts"][0][0] == llm.token_bos()
    assert len(eng.calls) == 3 and all(c["pooling"] == E.POOL_NONE and c["normalize"] is False for c in eng.calls)


@pytest.mark.parametrize("pt", [L.LLAMA_POOLING_TYPE_MEAN, L.LLAMA_POOLING_TYPE_CLS, L.LLAMA_POOLING_TYPE_LAST])
def test_pooled_shapes(pt):
    llm, eng = make(pooling_type=pt)
    n = len(llm.tokenize(b"hello world"))
    want = {L.LLAMA_POOLING_TYPE_CLS: row(0, 0), L.LLAMA_POOLING_TYPE_LAST: row(0, n - 1),
            L.LLAMA_POOLING_TYPE_MEAN: [float(v) for v in np.mean([row(0, t) for t in range(n)], axis=0,
                                                                  dtype=np.float32)]}[pt]
    one = llm.embed("hello world")
    assert len(one) == N_EMBD and all(isinstance(v, float) for v in one)
    assert one == pytest.approx(want, rel=1e-6)
    many = llm.embed(["hello world", "b c"])
    assert len(many) == 2 and many[0] == one and len(many[1]) == N_EMBD
    assert eng.calls[-1]["pooling"] == pt


def test_return_count():
    llm, _ = make(pooling_type=L.LLAMA_POOLING_TYPE_MEAN)
    texts = ["hello world", "a", "one two three"]
    total = sum(len(llm.tokenize(t.encode())) for t in texts)
    out, count = llm.embed(texts, return_count=True)
    assert count == total and out == llm.embed(texts)
    one, c1 = llm.embed("a", return_count=True)
    assert c1 == len(llm.tokenize(b"a")) and len(one) == N_EMBD


def test_truncation_to_n_batch_and_the_error_without_it():
    llm, eng = make(n_batch=4)
    assert llm.n_batch == 4
    text = "one two three four five six seven"
    toks = llm.tokenize(text.encode())
    assert len(toks) > 4
    out, count = llm.embed(text, return_count=True)
    assert len(out) == 4 and count == 4 and eng.calls[-1]["prompts"] == [toks[:4]]
    with pytest.raises(ValueError, match=rf"Requested tokens \({len(toks)}\) exceed batch size of 4"):
        llm.embed(text, truncate=False)
    assert len(eng.calls) == 1  # refused before anything reached the engine
    assert llm.embed("a", truncate=False) == [row(0, t) for t in range(len(llm.tokenize(b"a")))]
    big, _ = make(n_batch=4096)
    assert big.n_batch == 64  # min(n_batch, n_ctx)


def test_needs_embedding_true():
    llm, eng = make(embedding=False)
    with pytest.raises(RuntimeError, match="Llama model must be created with embedding=True to call this method"):
        llm.embed("hello")
    with pytest.raises(RuntimeError, match="embedding=True"):
        llm.create_embedding("hello")
    assert eng.calls == []


def test_create_embedding_dict():
    llm, _ = make(pooling_type=L.LLAMA_POOLING_TYPE_CLS)
    texts = ["hello world", "a"]
    total = sum(len(llm.tokenize(t.encode())) for t in texts)
    d = llm.create_embedding(texts)
    assert list(d) == ["object", "data", "model", "usage"]
    assert d["object"] == "list" and d["model"] == MODEL
    assert d["usage"] == {"prompt_tokens": total, "total_tokens": total}
    assert d["data"] == [{"object": "embedding", "embedding": row(0, 0), "index": 0},
                         {"object": "embedding", "embedding": row(1, 0), "index": 1}]
    one = llm.create_embedding("a", model="my-name")
    assert one["model"] == "my-name" and len(one["data"]) == 1 and one["data"][0]["index"] == 0
    assert one["data"][0]["embedding"] == row(0, 0)
    n = len(llm.tokenize(b"a"))
    assert one["usage"] == {"prompt_tokens": n, "total_tokens": n}
    # without pooling the embedding of an item is its per-token lists
    llm, _ = make()
    d = llm.create_embedding("a")
    assert d["data"][0]["embedding"] == [row(0, t) for t in range(n)]


def test_front_without_embeddings():
    llm, _ = make(eng=NoEmbedEngine())
    with pytest.raises(NotImplementedError):
        llm.embed("hello")
    # a front built before the embedding attributes existed (cls.__new__, no _embedding): the documented error
    bare = Llama.from_engine(MODEL, NoEmbedEngine(), n_ctx=64)
    for name in ("_embedding", "_pooling_type", "n_batch"):
        delattr(bare, name)
    assert bare.pooling_type() == L.LLAMA_POOLING_TYPE_NONE
    with pytest.raises(RuntimeError, match="embedding=True"):
        bare.embed("hello")


@pytest.mark.parametrize("bad", [4, 5, -2, 99])
def test_bad_pooling_type(bad):  # 4 = LLAMA_POOLING_TYPE_RANK
    with pytest.raises(ValueError, match="pooling_type"):
        make(pooling_type=bad)
    with pytest.raises(ValueError, match="pooling_type"):
        Llama(MODEL, embedding=True, pooling_type=bad)  # refused before any engine is created


def test_normalize_is_the_engines():
    llm, eng = make(pooling_type=L.LLAMA_POOLING_TYPE_LAST)
    n = len(llm.tokenize(b"hello world"))
    plain = llm.embed("hello world")
    normed = llm.embed("hello world", normalize=True)
    assert [c["normalize"] for c in eng.calls] == [False, True]
    assert plain == row(0, n - 1)
    assert normed == [-v for v in plain]  # exactly what the engine returned: the host did not rescale it
