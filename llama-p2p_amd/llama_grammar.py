"""``LlamaGrammar`` -- llama-cpp-python's grammar object for ``Llama.create_completion(grammar=)``.

    grammar = LlamaGrammar.from_string('root ::= ("yes" | "no") "."')
    llm.create_completion(prompt, grammar=grammar)

The grammar language is llama.cpp's GBNF.  The text is checked when the object is made: syntax
errors, undefined rules, a missing ``root``, ``{m,n}`` with ``n < m`` and left-recursive rules raise ``ValueError``
with the rule or position.  The matcher runs in the engine's library (csrc/grammar.cpp); a ``Llama`` compiles the
grammar once over its vocabulary and keeps the compiled form on this object.
"""
from __future__ import annotations

import os
import sys
import threading
import weakref
from typing import Any, Optional

from . import engine as _engine

# llama.cpp's grammars/json.gbnf
JSON_GBNF = r'''root   ::= object
value  ::= object | array | string | number | ("true" | "false" | "null") ws

object ::=
  "{" ws (
            string ":" ws value
    ("," ws string ":" ws value)*
  )? "}" ws

array  ::=
  "[" ws (
            value
    ("," ws value)*
  )? "]" ws

string ::=
  "\"" (
    [^"\\\x7F\x00-\x1F] |
    "\\" (["\\bfnrt] | "u" [0-9a-fA-F]{4}) # escapes
  )* "\"" ws

number ::= ("-"? ([0-9] | [1-9] [0-9]{0,15})) ("." [0-9]+)? ([eE] [-+]? [0-9] [1-9]{0,15})? ws

# Optional space: by convention, applied in this grammar after literal chars when allowed
ws ::= | " " | "\n" [ \t]{0,20}
'''

_check_vocab = None
_check_lock = threading.Lock()


def _syntax_check(text: str):
    """Compiles the text over a one-token vocabulary: everything GBNF refuses is refused here (ValueError)."""
    global _check_vocab
    with _check_lock:
        if _check_vocab is None:
            _check_vocab = _engine.GrammarVocab([b"a"], [])
        _engine.CompiledGrammar(_check_vocab, text, cache_entries=0).close()


class LlamaGrammar:
    def __init__(self, *args, _grammar: str, **kwargs):
        self._grammar = _grammar
        self._root = "root"
        _syntax_check(_grammar)
        self._compiled: "weakref.WeakKeyDictionary[Any, _engine.CompiledGrammar]" = weakref.WeakKeyDictionary()
        self._lock = threading.Lock()

    @classmethod
    def from_string(cls, grammar: str, verbose: bool = True) -> "LlamaGrammar":
        return cls(_grammar=grammar)

    @classmethod
    def from_file(cls, file: str, verbose: bool = True) -> "LlamaGrammar":
        try:
            with open(os.fspath(file), encoding="utf-8") as f:
                grammar = f.read()
        except Exception as err:
            raise Exception(f"{cls.from_file.__name__}: error reading grammar file: {err}")
        if grammar:
            return cls.from_string(grammar, verbose=verbose)
        raise ValueError(f"{cls.from_file.__name__}: error parsing grammar file: params_grammer is empty")

    @classmethod
    def from_json_schema(cls, json_schema: str, verbose: bool = True) -> "LlamaGrammar":
        raise NotImplementedError("from_json_schema is not supported; JSON_GBNF constrains the output to JSON")

    def compiled_for(self, owner, vocab: "_engine.GrammarVocab") -> "_engine.CompiledGrammar":
        """The grammar compiled over `vocab`, once per owner (a Llama) and kept while the owner lives."""
        with self._lock:
            g = self._compiled.get(owner)
            if g is None:
                g = self._compiled[owner] = _engine.CompiledGrammar(vocab, self._grammar)
            return g
