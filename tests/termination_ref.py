"""What test_termination_host.py and test_termination_gpu.py share: the prompt pool, how an end-of-generation
token is chosen from recorded outputs, what a stopping request must return, and the host replay of a speculating
request's schedule.  Nothing here touches the GPU.
"""
import numpy as np

MODELS = ["test-tiny", "test-d128"]
N_CTX = 128
T = 24  # max_tokens of every request
N_POOL = 24
# where EOS falls in a lone request's output: round 1 of the scheduler produces out[1..8], round 2 out[9..16] --
# 0: the prefill's pick (admission); 1, 9: first step of a round; 4: mid-round; 8, 16: last step of a round;
# 23: the token that also reaches max_tokens
STOP_INDICES = [0, 1, 4, 8, 9, 16, 23]


def vocab(name):
    from llama_p2p_amd import synth

    return synth.SHAPES[name].n_vocab


def pool(name):
    """N_POOL prompts: BOS + 3..39 random ids from [3, n_vocab) -- never the BOS / default EOS ids inside."""
    rng = np.random.default_rng(2024)
    V = vocab(name)
    return [[1] + [int(t) for t in rng.integers(3, V, int(rng.integers(3, 40)))] for _ in range(N_POOL)]


def candidates(outputs, j, prompts=None):
    """(prompt index, E) pairs with E's first occurrence in outputs[p] at index j; E absent from the prompt itself
    when `prompts` is given (a request never sees its own EOS in its input)."""
    found = []
    for p, out in enumerate(outputs):
        out = list(out)
        if j < len(out) and out[j] not in out[:j] and (prompts is None or out[j] not in prompts[p]):
            found.append((p, int(out[j])))
    return found


def choose_stops(outputs, prompts=None, indices=STOP_INDICES, prefer=()):
    """{j: (prompt index, E)} for every j that has a candidate; among the candidates an E of `prefer` or one
    already chosen for another j comes first, so that few distinct E (model files) are needed."""
    chosen = {}
    for j in indices:
        c = candidates(outputs, j, prompts)
        if not c:
            continue
        have = set(prefer) | {e for _, e in chosen.values()}
        chosen[j] = next((pe for pe in c if pe[1] in have), c[0])
    return chosen


def expectation(ref, E, finish_stop=1, finish_length=0, n=T):
    """Tokens and finish reason of a request that stops at E, from its ignore_eos output `ref`: the EOS token is
    returned, and the EOS test comes before the max_tokens test."""
    ref = [int(t) for t in ref[:n]]
    if E in ref:
        return ref[:ref.index(E) + 1], finish_stop
    return ref, finish_length


def most_frequent(outputs, avoid=()):
    """The token most outputs contain (ties: the lowest id), so that a batch's rows stop at many different steps."""
    count = {}
    for out in outputs:
        for t in set(int(x) for x in out):
            count[t] = count.get(t, 0) + 1
    return min((t for t in count if t not in avoid), key=lambda t: (-count[t], t))


def absent_token(outputs, n_vocab, avoid=()):
    """The lowest id >= 3 that no output holds."""
    seen = {int(t) for out in outputs for t in out} | set(avoid)
    return next(t for t in range(3, n_vocab) if t not in seen)


def replay_spec(prompt, out, D, NG):
    """The speculating schedule of a lone request replayed on the host over the tokens it kept: one entry
    (index in `out` of the step's first token, drafted, accepted) per step.  out[0] comes from the prefill.  A step
    keeps its matching draft tokens and one more; the engine counts `kept - 1` of a step as accepted, and a step's
    kept tokens end where `out` ends, so in the last step only the tokens up to EOS (or max_tokens) count."""
    from llama_p2p_amd.speculative import LlamaPromptLookupDecoding

    look = LlamaPromptLookupDecoding(max_ngram_size=NG, num_pred_tokens=D)
    steps, m = [], 1
    while m < len(out):
        d = look(np.asarray(list(prompt) + list(out[:m]), dtype=np.intc)).tolist()
        a = 0
        while a < len(d) and m + a < len(out) and d[a] == out[m + a]:
            a += 1
        kept = min(a + 1, len(out) - m)  # the correction token after the run is dropped when the run ends at EOS
        steps.append((m, len(d), kept - 1))
        m += kept
    return steps
