"""The Q8_0 KV cache's public interface, without a GPU: Llama(type_k=, type_v=, flash_attn=),
Engine(kv_type=), mx_opts.kv_type and the probe's export."""
import inspect

import pytest

from llama_p2p_amd import engine as E
from llama_p2p_amd.llama import Llama


def test_llama_signature():
    p = inspect.signature(Llama.__init__).parameters
    for name, default in (("type_k", None), ("type_v", None), ("flash_attn", False)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is default, name


def test_engine_signature_and_opts_default():
    assert inspect.signature(E.Engine.__init__).parameters["kv_type"].default == 1
    o = E.MxOpts()
    o.kv_type = 77
    E.lib().mx_opts_default(o)
    assert o.kv_type == 1 and E.MxOpts._fields_[-1][0] == "kv_type"


@pytest.mark.parametrize("kw", [dict(type_k=2), dict(type_k=8, type_v=1), dict(type_v=8), dict(type_k=8, type_v=30)])
def test_unsupported_types_raise_before_the_model_is_opened(kw):
    with pytest.raises(NotImplementedError, match="Q8_0"):
        Llama("/nonexistent/model.gguf", **kw)  # a missing file would be a ValueError: the types are checked first


def test_probe_is_exported():
    assert "mx_attention_kvq_probe" in E.EXPORTS and hasattr(E.lib(), "mx_attention_kvq_probe")
