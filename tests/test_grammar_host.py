"""Grammar matcher on the host: csrc/grammar.cpp through the C ABI against tests/grammar_ref.py, an
Earley recogniser written from the semantics.  Every comparison is of integers: the product's mask equals the
reference's allowed set in every token, at every step of seeded random walks.  No GPU.

    python tests/test_grammar_host.py DIR

writes the vocabularies and the table's grammars to DIR for tools/grammar_selfcheck.cpp.
"""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from grammar_ref import RefGrammar  # noqa: E402

WALK_STEPS = 64

ARITH = r'''
root ::= expr
expr ::= term (("+" | "-") expr)?      # right recursion
term ::= factor (("*" | "/") term)?
factor ::= num | "(" expr ")" | "-" factor
num ::= [0-9]+
'''
GRAMMARS = {
    "json": None,  # JSON_GBNF, filled in below
    "arith": ARITH,
    "negated": 'root ::= [^a-z0-9 ]+ "." [^.]* "!"\n',
    "dot": 'root ::= . . "a" .* "."\n',
    "reps": 'root ::= ("ab"){2} "," ("c" | "d"){2,} "," ([0-9] "x"){1,3} "," ("y")? ("z" | "Z")* ("!")+\n',
    "nullable": 'root ::= a b c "."\na ::= "a"?\nb ::= ("b" b)?\nc ::= a | \n',
    "ambiguous": 'root ::= ("a" | "a" "a" | "aa") * tail\ntail ::= ("ab" | "a" "b") ("." | "!")\n',
    "unicode": 'root ::= ([à-ÿ] | [一-龥] | [\\U0001F600-\\U0001F64F] | "é" | " ")+ "."\n',
    "bounded": 'root ::= ("yes" | "no") " " [a-z]{3,5} "."\n',
}


def _json():
    from llama_p2p_amd.llama_grammar import JSON_GBNF

    return JSON_GBNF


def grammar_text(name):
    return _json() if name == "json" else GRAMMARS[name]


def spm_vocab():
    from llama_p2p_amd.gguf import synthetic_spm_vocab
    from llama_p2p_amd.tokenizer import Tokenizer

    toks, scores, types = synthetic_spm_vocab(512)
    tk = Tokenizer(toks, scores, types, "llama", bos_id=1, eos_id=2)
    return [tk.token_to_piece(t) for t in range(512)], [t for t in range(512) if tk.is_eog(t)]


def hand_vocab():
    """Multi-code-point pieces, a piece that ends inside a UTF-8 sequence, an invalid one, empty ones, two
    end-of-generation ids, no byte tokens."""
    pieces = [b"", b"<eos>", b"", b"<eot>"]  # 1 and 3: end of generation
    pieces += [bytes([c]) for c in b"abcdxyzZ0123456789+-*/().,!?\"{}[]:\\ \n\tetrufalsn"]
    pieces += [b"ab", b"aa", b"abab", b"true", b"false", b"null", b"yes", b"no", b" a", b"12", b"\": ", b"{\"", b"\"}",
               b"ye", b"s ", b"xyz", b"xy.", b"))", b"(("]
    pieces += ["é".encode(), "à".encode(), "ÿ".encode(), "一".encode(), "龥".encode(), "中文".encode(),
               "😀".encode(), "é é".encode(), "\u00e9.".encode(), "中".encode()[:2], "中".encode()[2:],
               "😀".encode()[:1], "😀".encode()[1:3], "😀".encode()[3:], b"a\xc3", b"\xa9", b"\xe4\xb8",
               b"\xff", b"\xc3\x28", b"\xc0\x80", b"\xed\xa0\x80", b"a\x80"]
    return pieces, [1, 3]


VOCABS = {"spm": spm_vocab, "hand": hand_vocab}
_cache = {}


def vocab(name):
    if name not in _cache:
        from llama_p2p_amd import engine as E

        pieces, eog = VOCABS[name]()
        _cache[name] = (pieces, eog, E.GrammarVocab(pieces, eog))
    return _cache[name]


def walk(gname, vname, seed, cache_entries=None, check=True):
    """A seeded random walk of up to WALK_STEPS accepted tokens; returns (tokens, masks, pending byte counts)."""
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab(vname)
    g = E.CompiledGrammar(gv, grammar_text(gname), cache_entries=cache_entries)
    ref = RefGrammar(grammar_text(gname)) if check else None
    st = g.state()
    rng = np.random.default_rng(seed)
    gen, toks, masks, pend = b"", [], [], set()
    for step in range(WALK_STEPS):
        got = st.allowed()
        masks.append(got.copy())
        if check:
            want = np.array(ref.allowed(pieces, eog, gen), dtype=bool)
            diff = np.nonzero(got != want)[0]
            assert diff.size == 0, (f"{gname}/{vname} seed {seed} step {step} after {gen!r}: tokens {diff[:8].tolist()} "
                                    f"(pieces {[pieces[t] for t in diff[:8]]}) product {got[diff[:8]].tolist()}")
            assert st.may_end() == ref.may_end(gen)
            pend.add(len(ref.split(gen)[1]))
        ids = np.nonzero(got)[0]
        if ids.size == 0:
            break
        # end-of-generation ids rarely, so that walks go on where the grammar may end but need not
        body = [t for t in ids if t not in eog]
        t = int(rng.choice(body)) if body and rng.random() < 0.9 else int(rng.choice(ids))
        st.accept(t)
        toks.append(t)
        if t in eog:
            break
        gen += pieces[t]
    return toks, masks, pend, g


@pytest.mark.parametrize("vname", ["spm", "hand"])
@pytest.mark.parametrize("gname", sorted(GRAMMARS))
def test_mask_equals_reference_on_random_walks(gname, vname):
    pend = set()
    for seed in range(3):
        toks, masks, p, g = walk(gname, vname, seed)
        assert toks, "the walk accepted no token"
        pend |= p
    if gname == "unicode" and vname == "spm":  # only byte tokens spell these: every pending length occurs
        assert {1, 2, 3} <= pend, pend


@pytest.mark.parametrize("gname", ["json", "arith", "unicode"])
def test_walks_hit_the_cache_and_masks_do_not_depend_on_it(gname):
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("spm")
    g = E.CompiledGrammar(gv, grammar_text(gname))
    runs = []
    for rnd in range(2):  # the same walk twice over one compiled grammar
        st, rng, masks = g.state(), np.random.default_rng(5), []
        for _ in range(WALK_STEPS):
            m = st.allowed()
            masks.append(m)
            ids = [t for t in np.nonzero(m)[0] if t not in eog]
            if not ids:
                break
            st.accept(int(rng.choice(ids)))
        runs.append(masks)
        if rnd == 0:
            first = g.cache_stats()
    both = E.Engine.grammar_cache_stats(g)
    assert first["misses"] >= 1 and first["entries"] == first["misses"]
    assert both["misses"] == first["misses"], "the replay computed a mask again"
    assert both["hits"] >= first["hits"] + len(runs[1])
    assert all((a == b).all() for a, b in zip(*runs))
    _, nocache, _, g0 = walk(gname, "spm", 5, cache_entries=0, check=False)
    _, cached, _, _ = walk(gname, "spm", 5, check=False)
    assert g0.cache_stats() == {"hits": 0, "misses": len(nocache), "entries": 0}
    assert len(nocache) == len(cached) and all((a == b).all() for a, b in zip(nocache, cached))


def test_cache_is_bounded_lru():
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("spm")
    g = E.CompiledGrammar(gv, grammar_text("arith"), cache_entries=2)
    st = g.state()
    for t in [pieces.index(b"1"), pieces.index(b"+"), pieces.index(b"("), pieces.index(b"2")]:
        st.mask()
        st.accept(t)
    assert g.cache_stats()["entries"] == 2


BAD = {
    "no_assign": 'root "a"\n',
    "unterminated_string": 'root ::= "abc\n',
    "unterminated_class": 'root ::= [abc\n',
    "unclosed_group": 'root ::= ("a" | "b"\n',
    "stray_close": 'root ::= "a")\n',
    "bad_escape": 'root ::= "\\q"\n',
    "bad_hex": 'root ::= "\\xZZ"\n',
    "repeat_nothing": 'root ::= * "a"\n',
    "bad_count": 'root ::= "a"{x}\n',
    "unclosed_count": 'root ::= "a"{2,3\n',
    "two_rules_one_line": 'root ::= a b ::= "c"\na ::= "a"\n',
    "defined_twice": 'root ::= "a"\nroot ::= "b"\n',
    "empty_name": '::= "a"\n',
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_syntax_errors_are_refused(name):
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match=r"line \d+, column \d+"):
        LlamaGrammar.from_string(BAD[name])


def test_undefined_rule_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match="undefined rule 'item'.*'list'"):
        LlamaGrammar.from_string('root ::= list\nlist ::= item+\n')


def test_missing_root_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match="no 'root' rule"):
        LlamaGrammar.from_string('start ::= "a"\n')


def test_count_with_n_below_m_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match=r"\{3,2\}.*n < m.*'root'"):
        LlamaGrammar.from_string('root ::= "a"{3,2}\n')


def test_direct_left_recursion_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match="'expr' is left-recursive"):
        LlamaGrammar.from_string('root ::= expr\nexpr ::= expr "+" [0-9] | [0-9]\n')


def test_indirect_left_recursion_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match="is left-recursive"):
        LlamaGrammar.from_string('root ::= a\na ::= b "x" | "y"\nb ::= c\nc ::= (a "z")\n')


def test_left_recursion_through_a_nullable_prefix_is_refused():
    from llama_p2p_amd.llama_grammar import LlamaGrammar

    with pytest.raises(ValueError, match="'a' is left-recursive"):
        LlamaGrammar.from_string('root ::= a\na ::= ws opt a "x" | "y"\nws ::= " "*\nopt ::= "o"?\n')
    LlamaGrammar.from_string('root ::= a\na ::= ws "(" a ")" | "y"\nws ::= " "*\n')  # right of a terminal: fine


def test_dead_end_reports_an_empty_mask():
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("hand")
    g = E.CompiledGrammar(gv, 'root ::= "a" "#"\n')  # no piece holds '#'
    st = g.state()
    w, status = st.mask()
    assert status == E.GRAMMAR_OK and w.any()
    st.accept(pieces.index(b"a"))
    w, status = st.mask()
    assert status == E.GRAMMAR_DEAD_END and not w.any() and not st.may_end()
    with pytest.raises(E.MxError):
        st.accept(pieces.index(b"a"))
    ref = RefGrammar('root ::= "a" "#"\n')
    assert not any(ref.allowed(pieces, eog, b"a"))


def test_position_cap_is_reported_not_looped_on():
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("hand")
    # after n 'a's the closing letters still owed are any of 2^n sequences: one position each
    g = E.CompiledGrammar(gv, 'root ::= s\ns ::= "a" s "b" | "a" s "c" | "a"\n')
    st, a = g.state(), pieces.index(b"a")
    status = E.GRAMMAR_OK
    for n in range(16):
        w, status = st.mask()
        if status != E.GRAMMAR_OK:
            break
        st.accept(a)
    assert status == E.GRAMMAR_CAP and not w.any(), (n, status)
    # 2^12 = 4096; the walk of the vocabulary also passes through the sets behind "aa" and "abab", so the cap is met
    # a few tokens before the state's own set reaches it
    assert 8 <= n <= 12
    w, status = st.mask()
    assert status == E.GRAMMAR_CAP


HEAVY = {  # legal, not left-recursive, never near 4096 positions -- and quadratic or worse for a matcher that
    # expands every stack of a set on its own: minutes to hours per mask before the work was shared and budgeted
    25: 'root ::= ([a-z]? [a-z]? [a-z]? [a-z]? [a-z]? [a-z]?){0,25} "."\n',
    200: 'root ::= ([a-z]? [a-z]? [a-z]? [a-z]? [a-z]? [a-z]?){0,200} "."\n',
    600: 'root ::= ([a-z]? [a-z]? [a-z]? [a-z]? [a-z]? [a-z]?){0,600} "."\n',
}
# a mask may touch 2^20 stack elements (csrc/grammar.h WORK_BUDGET), about 60 ms of one core; the bound asserted
# leaves a slow, shared machine a factor of 30
MASK_SECONDS = 2.0


@pytest.mark.parametrize("K", sorted(HEAVY))
def test_mask_time_is_bounded_by_the_work_budget(K):
    import time

    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("spm")
    st = E.CompiledGrammar(gv, HEAVY[K], cache_entries=0).state()
    a = pieces.index(b"a")
    for step in range(3):
        t0 = time.perf_counter()
        w, status = st.mask()
        dt = time.perf_counter() - t0
        print(f"K {K} step {step}: status {status}, {1e3 * dt:.1f} ms")
        assert dt < MASK_SECONDS
        if K == 25:  # 150 positions: inside the budget, and right
            assert status == E.GRAMMAR_OK
            ref = RefGrammar(HEAVY[K])
            assert (st.allowed() == np.array(ref.allowed(pieces, eog, b"a" * step), dtype=bool)).all()
            st.accept(a)
        else:  # 1200 and 3600 positions: under the position cap, past the work budget -- reported, not computed
            assert status == E.GRAMMAR_CAP and not w.any()
            break


def test_many_small_positions_stay_cheap():
    """x{0,2000} with x ::= [a-z] y{0,20}: thousands of helper rules, a handful of positions per state."""
    import time

    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("spm")
    st = E.CompiledGrammar(gv, 'root ::= x{0,2000}\nx ::= [a-z] y{0,20}\ny ::= [0-9]\n', cache_entries=0).state()
    a, worst = pieces.index(b"a"), 0.0
    for step in range(40):
        t0 = time.perf_counter()
        w, status = st.mask()
        worst = max(worst, time.perf_counter() - t0)
        assert status == E.GRAMMAR_OK and w.any()
        st.accept(a)
    print(f"worst mask {1e3 * worst:.2f} ms")
    assert worst < MASK_SECONDS


def test_long_repetition_chain_of_nullable_items_ends():
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("hand")
    g = E.CompiledGrammar(gv, 'root ::= ("a"?){0,10000} "."\n')  # one position per count still open: over the cap
    w, status = g.state().mask()
    assert status == E.GRAMMAR_CAP and not w.any()
    with pytest.raises(ValueError, match="too large"):
        E.CompiledGrammar(gv, 'root ::= "a"{100000}\n')


def test_destroy_while_in_use_and_shared_states():
    from llama_p2p_amd import engine as E

    pieces, eog = hand_vocab()
    gv = E.GrammarVocab(pieces, eog)
    g = E.CompiledGrammar(gv, grammar_text("bounded"))
    s1, s2 = g.state(), g.state()
    gv.close()  # the grammar keeps the vocabulary, the states keep the grammar
    g.close()
    y, n = pieces.index(b"yes"), pieces.index(b"no")
    s1.accept(y)
    assert s2.allowed()[n] and not s1.allowed()[n]  # two states, one grammar, independent places
    s2.accept(n)
    sp = pieces.index(b" ")
    assert s1.allowed()[sp] and s2.allowed()[sp] and int(s1.allowed().sum()) == 2  # " " and " a"
    s1.close()
    assert s2.allowed()[sp]
    s2.close()


def test_end_of_generation_only_where_the_grammar_may_end():
    from llama_p2p_amd import engine as E

    pieces, eog, gv = vocab("hand")
    st = E.CompiledGrammar(gv, 'root ::= "é" "."?\n').state()
    assert not st.may_end() and not st.allowed()[eog].any()
    st.accept(pieces.index("é".encode()))
    m = st.allowed()
    assert st.may_end() and m[eog].all() and m[pieces.index(b".")] and int(m.sum()) == 3
    st.accept(3)
    assert st.mask()[1] == E.GRAMMAR_DEAD_END  # ended: nothing follows


def test_llama_grammar_round_trips(tmp_path):
    from llama_p2p_amd.llama_grammar import JSON_GBNF, LlamaGrammar

    g = LlamaGrammar.from_string(JSON_GBNF, verbose=False)
    assert g._grammar == JSON_GBNF
    p = tmp_path / "g.gbnf"
    p.write_text(grammar_text("unicode"), encoding="utf-8")
    assert LlamaGrammar.from_file(str(p))._grammar == grammar_text("unicode")
    (tmp_path / "empty.gbnf").write_text("")
    with pytest.raises(ValueError):
        LlamaGrammar.from_file(str(tmp_path / "empty.gbnf"))
    with pytest.raises(Exception):
        LlamaGrammar.from_file(str(tmp_path / "missing.gbnf"))
    with pytest.raises(NotImplementedError):
        LlamaGrammar.from_json_schema("{}")


def test_greedy_cases_are_decided_on_the_oracle(oracle_mod):
    """The contexts tests/test_grammar_gpu.py judges greedy picks on: along the masked greedy path of the CPU
    oracle at most 5 % of the steps have their two best allowed logits within the tolerance (here: none)."""
    import grammar_ref as R
    from llama_p2p_amd import engine as E
    from llama_p2p_amd import synth

    pieces, eog, gv = vocab("spm")
    om = oracle_mod.OracleModel(synth.SHAPES["test-tiny"], seed=0)
    steps = close = 0
    for text, seed in R.GREEDY_CASES:
        st, prompt = E.CompiledGrammar(gv, text).state(), R.greedy_prompt(seed)
        ctx = om.context(64)
        row, pos = ctx.eval(np.array(prompt, np.int32), 0)[0], len(prompt)
        for _ in range(R.GREEDY_MAX_TOKENS):
            t, gap = R.masked_top2(row, st.allowed())
            steps += 1
            close += gap <= R.greedy_tol(row)
            st.accept(t)
            if t in eog:
                break
            row, pos = ctx.eval(np.array([t], np.int32), pos)[0], pos + 1
        assert t in eog, "the grammar did not end within GREEDY_MAX_TOKENS"
    print(f"{steps} steps, {close} within the tolerance")
    assert steps >= 60 and close <= 0.05 * steps


def test_exports():
    from llama_p2p_amd import engine as E

    for name in ("mx_vocab_create", "mx_vocab_destroy", "mx_grammar_create", "mx_grammar_destroy",
                 "mx_grammar_state_create", "mx_grammar_state_mask", "mx_grammar_state_accept",
                 "mx_grammar_state_may_end", "mx_grammar_state_destroy", "mx_grammar_cache_stats", "mx_submit_grammar",
                 "mx_grammar_mask_probe"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
    assert E.Engine.supports_grammar


def dump_vocab(path, pieces, eog):
    """The vocabulary file tools/grammar_selfcheck.cpp reads: 'MXGV', n_vocab, n_eog (u32), the ids (i32), the
    offsets (u64 [n_vocab + 1]), the piece bytes."""
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
    with open(path, "wb") as f:
        f.write(b"MXGV" + struct.pack("<II", len(pieces), len(eog)))
        f.write(np.asarray(eog, dtype=np.int32).tobytes() + off.tobytes() + b"".join(pieces))


def test_selfcheck_tool_reads_the_dump_and_passes(tmp_path):
    """tools/grammar_selfcheck.cpp (csrc/grammar.cpp alone, the program a host sanitizer build runs) built plainly
    here: it reads what dump_vocab writes and every one of its checks holds."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    for vn, fn in VOCABS.items():
        dump_vocab(tmp_path / (vn + ".vocab"), *fn())
    for gn in ("json", "arith", "unicode", "bounded"):
        (tmp_path / (gn + ".gbnf")).write_text(grammar_text(gn), encoding="utf-8")
    exe = str(tmp_path / "grammar_selfcheck")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(root, "tools", "grammar_selfcheck.cpp"),
                    os.path.join(root, "llama-p2p_amd", "csrc", "grammar.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "all checks passed" in p.stdout, p.stdout[-2000:]
    assert p.stdout.count(" masks ") == 2 * 4 * 4  # vocabularies x grammars x seeds


if __name__ == "__main__":
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for vn, fn in VOCABS.items():
        dump_vocab(os.path.join(out, vn + ".vocab"), *fn())
    for gn in GRAMMARS:
        with open(os.path.join(out, gn + ".gbnf"), "w", encoding="utf-8") as f:
            f.write(grammar_text(gn))
