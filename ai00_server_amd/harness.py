"""Mirror of the ai00-core code that *calls* the hot path (crates/ai00-core/src/run.rs), for tests and benches.

    InferLoop.run_pending     the `infer` task        run.rs:1072-1162  (per-slot FIFO, one request per slot per
                                                       step, loop until the RnnInput is consumed)
    greedy_process            `process` decode loop   run.rs:788-1020   with the arg-max sampler (Nucleus top_k=1,
                                                       sampler/nucleus.rs:77-89) and token 0 = stop (run.rs:855)
    perplexity                `perplexity`            run.rs:699-755    (RnnOption::Full consumer)
    perplexity_scored         the same request with the realised tokens scored on the device (`Runtime.infer_score`)
    generate_resident         the decode loop of one request in resident generation (`Runtime.gen_run`), with `top_logprobs` the
                              `logprobs` object of an OpenAI-style completion: per token (token, logp, [(id, logp) ...])
    ReplicaRouter             SURVEY 8(e)             request-level sharding over N independent engines (no collective)

Works against anything that has `.max_batch`, `.infer(RnnInput)` and `.state` like `runtime.Runtime`.
"""
from __future__ import annotations

import math
from collections import deque
from dataclasses import dataclass, field

import numpy as np

from .runtime import SCORE_SKIP, TOPN_NONE, GenCapture, RnnInput, RnnInputBatch, RnnOption


@dataclass
class InferRequest:            # InferBatch::Run {batch, tokens, option, sender}  run.rs:1091-1098
    batch: int
    tokens: list
    option: RnnOption = RnnOption.Last
    outputs: list = field(default_factory=list)     # what `sender` would receive: one array per emitting infer call


class InferLoop:
    """The single consumer of InferBatch messages (run.rs:1072-1162)."""

    def __init__(self, runtime):
        self.rt = runtime
        self.queues: dict[int, deque] = {}

    def submit(self, req: InferRequest) -> InferRequest:          # schedule(): Run -> per-slot VecDeque
        self.queues.setdefault(req.batch, deque()).append(req)
        return req

    def run_pending(self) -> int:
        """`while batches.values().map(len).sum() > 0 { ... }` (run.rs:1120-1157). Returns #infer calls."""
        calls = 0
        while sum(len(q) for q in self.queues.values()) > 0:
            inference = [RnnInputBatch() for _ in range(self.rt.max_batch)]
            senders: dict[int, InferRequest] = {}
            for b, q in self.queues.items():                      # pop <= 1 request per slot (run.rs:1124-1130)
                if not q:
                    continue
                req = q.popleft()
                inference[b] = RnnInputBatch(list(req.tokens), req.option)
                senders[b] = req
            inp = RnnInput(inference)
            while inp.num_token() > 0:                            # run.rs:1134-1156
                inp, out = self.rt.infer(inp)
                calls += 1
                for b, o in enumerate(out):
                    if len(o) and b in senders:
                        senders[b].outputs.append(o)
        return calls


def greedy_process(loop: InferLoop, batch: int, prompt, max_tokens: int) -> list[int]:
    """Decode loop of one slot with the arg-max sampler; empty prompt => [0] (run.rs:489-492); token 0 stops."""
    tokens = list(prompt) if len(prompt) else [0]
    out = []
    for _ in range(max_tokens):
        req = loop.submit(InferRequest(batch, tokens, RnnOption.Last))
        loop.run_pending()
        logits = req.outputs[-1][-1]
        tok = int(np.argmax(logits))
        if tok == 0:                                              # run.rs:855
            break
        out.append(tok)
        tokens = [tok]
    return out


def perplexity(loop: InferLoop, batch: int, tokens, head: float | None = None) -> float:
    """run.rs:699-755: Full outputs, softmax without max-subtraction, ppl = -sum(ln p) / len(tokens')."""
    p = []
    toks = list(tokens) if head is not None else [0] + list(tokens)
    n = len(tokens)
    if head is not None:
        p.append(head)
    req = loop.submit(InferRequest(batch, toks, RnnOption.Full))
    loop.run_pending()
    index = 1
    for chunk in req.outputs:                                     # one array per infer call, split(1) per token
        for row in chunk:
            if len(p) >= n:
                break
            if index < len(toks):
                e = np.exp(row.astype(np.float32))
                p.append(float(e[toks[index]] / e.sum(dtype=np.float32)))
            index += 1
    return float(-sum(math.log(x) for x in p) / len(toks))


def perplexity_scored(loop_or_runtime, batch: int, tokens, head: float | None = None) -> float:
    """`perplexity` with the realised tokens scored on the device (`Runtime.infer_score`, rwkv_infer_score): tokens' = [0] + tokens, or
    tokens when `head` (the probability of tokens[0]) is given; every row's target is the next token, the last row is `SCORE_SKIP`;
    ppl = -(sum ln p [+ ln head]) / len(tokens').  4 bytes per token come back instead of a logits row.  Takes an `InferLoop` (whose
    queues must be drained) or a runtime.  Unlike `perplexity` — and run.rs:737-740 — the device subtracts the row maximum before it
    exponentiates, so logits beyond ~88 still score finitely; where `perplexity` is finite the two agree to fp32."""
    rt = getattr(loop_or_runtime, "rt", loop_or_runtime)
    toks = list(tokens) if head is not None else [0] + list(tokens)
    targets = [None] * rt.max_batch
    targets[batch] = toks[1:] + [SCORE_SKIP]
    inp = RnnInput([RnnInputBatch(toks if b == batch else [], RnnOption.Full) for b in range(rt.max_batch)])
    acc = math.log(head) if head is not None else 0.0
    while inp.num_token() > 0:
        inp, targets, scores = rt.infer_score(inp, targets)
        lp = np.asarray(scores[batch], dtype=np.float64)
        if not len(inp.batches[batch].tokens):                    # the request's last row is the skipped one
            lp = lp[:-1]
        acc += float(lp.sum())
    return float(-acc / len(toks))


def generate_resident(runtime, slot: int, prompt, max_tokens: int, sampler, seed: int = 0, stop_tokens=(), top_logprobs: int = 0,
                      steps_per_run: int = 16, constraint=None, halt: int = 0, capture=GenCapture(0), item=None):
    """One request through resident generation: `slot` is armed with the whole `prompt` (`Runtime.gen_arm_prompt`; `sampler` is the host
    sampler right after `init(prompt)`) and run until it finishes; nothing but token ids and a few numbers cross PCIe.  Returns one
    (token, prob) per emitted token; with `top_logprobs` = n > 0 (`Runtime.gen_set_topn`) one (token, logp, [(id, logp), ...]) instead:
    the token's ln-probability and the n most likely alternatives of the RAW model row (before penalties, bias and temperature), most
    likely first, as an OpenAI-style `logprobs` object lists them.  Other armed slots ride along; their tokens are dropped here.
    `constraint` is a `runtime.Dfa` or a `runtime.Pda` (`Pda.json(...)` for "answer in JSON"), set from its start with halt mode `halt`;
    it needs the token table (`Runtime.gen_set_token_bytes`).
    The prefix cache (run.rs:809-810, 834-845, 995-1001): with `item` (a `runtime.GenItem` that holds the whole prompt) the slot is armed by
    `Runtime.gen_arm_item` — no prefill, the first token is drawn from the item's row — and `prompt` is only the sampler's history.  With
    `capture` (`GenCapture.Prompt`, `.Finish` or both; `Prompt` needs a prompt to run, so not with `item`) the call returns
    (out, {flag: GenItem}) with the items the slot made."""
    if item is not None:
        runtime.gen_arm_item(slot, item, max_tokens, sampler, seed=seed, stop_tokens=stop_tokens)
    else:
        runtime.gen_arm_prompt(slot, prompt, max_tokens, sampler, seed=seed, stop_tokens=stop_tokens)
    capture = GenCapture(capture)
    if capture:
        runtime.gen_set_capture(slot, capture)
    if constraint is not None:
        if hasattr(constraint, "max_depth"):
            runtime.gen_set_pda(slot, constraint, halt=halt)
        else:
            runtime.gen_set_constraint(slot, constraint, halt=halt)
    if top_logprobs:
        runtime.gen_set_topn(slot, top_logprobs)
    out = []
    while True:
        res = runtime.gen_run(steps_per_run, top=top_logprobs)
        toks, probs, finish = res[0], res[1], res[3]
        for k in range(steps_per_run):
            if toks[k, slot] == 0xFFFFFFFF:
                continue
            if not top_logprobs:
                out.append((int(toks[k, slot]), float(probs[k, slot])))
                continue
            tok_logp, ids, lp = res[4][k, slot], res[5][k, slot], res[6][k, slot]
            out.append((int(toks[k, slot]), float(tok_logp), [(int(i), float(v)) for i, v in zip(ids, lp) if i != TOPN_NONE]))
        if finish[slot]:
            if not capture:
                return out
            return out, {flag: runtime.gen_take_item(slot, flag) for flag in (GenCapture.Prompt, GenCapture.Finish) if capture & flag}


def generate_resident_stream(runtime, slot: int, prompt, max_tokens: int, sampler, seed: int = 0, stop_tokens=(), top_logprobs: int = 0,
                             steps_per_run: int = 1024, constraint=None, halt: int = 0):
    """`generate_resident` as a GENERATOR that yields every (token, prob) as it is drawn (run.rs:1009), not when the run returns: a worker
    thread sits in `Runtime.gen_run` with a large `steps_per_run` (ctypes releases the GIL there) and this thread reads the records of a
    watch (`Runtime.gen_watch_open`).  It yields exactly the list `generate_resident` returns.  Closing the generator early cancels the
    slot (`GenWatch.cancel`, run.rs:934-935): it ends with `GenFinish.Cancelled` in the first step that sees the flag.
    The engine's watch is opened here and closed when the generator ends; top-n lists are not published, so `top_logprobs` must be 0."""
    import threading
    import time
    if top_logprobs:
        raise ValueError("a watch does not publish top-n lists: use generate_resident")
    runtime.gen_arm_prompt(slot, prompt, max_tokens, sampler, seed=seed, stop_tokens=stop_tokens)
    if constraint is not None:
        if hasattr(constraint, "max_depth"):
            runtime.gen_set_pda(slot, constraint, halt=halt)
        else:
            runtime.gen_set_constraint(slot, constraint, halt=halt)
    watch = runtime.gen_watch_open(min(max(int(steps_per_run), 1024), 65536))
    done, failure = threading.Event(), []

    def work():
        try:
            while not runtime.gen_run(steps_per_run)[3][slot]:
                pass
        except BaseException as e:                                    # handed to the consumer below
            failure.append(e)
        finally:
            done.set()

    worker = threading.Thread(target=work, name="gen_run", daemon=True)
    worker.start()
    try:
        finished = False
        while not finished:
            drained = done.is_set()                                   # looked at BEFORE the read: a record published behind it is seen next time
            toks, probs, fin, lost = watch.read(64)
            if lost:
                raise RuntimeError(f"the reader fell {lost} records behind the watch's ring")
            for k in range(len(toks)):
                if toks[k, slot] != 0xFFFFFFFF:
                    yield int(toks[k, slot]), float(probs[k, slot])
                if fin[k, slot]:
                    finished = True
                    break
            if len(toks) == 0:
                if drained:
                    break
                time.sleep(0.0002)
    finally:
        if worker.is_alive():
            watch.cancel(slot)                                        # closed early (or failed): the request is gone
        worker.join()
        watch.close()
    if failure:
        raise failure[0]


class NucleusSampler:
    """Host-side STATE of `NucleusSampler` (sampler/nucleus.rs:13-122) for the on-device sampling front-end: the
    penalty map lives here, its effect reaches the device as sparse logit adjustments (`adjustments()`), and the
    token the device picked is fed back through `update()` (nucleus.rs:104-119)."""

    def __init__(self, top_p=0.5, top_k=128, temperature=1.0, presence_penalty=0.3, frequency_penalty=0.3,
                 penalty_decay=0.99654026, bias: dict | None = None):
        self.top_p, self.top_k, self.temperature = float(top_p), int(top_k), float(temperature)
        self.ap, self.af, self.ad = np.float32(presence_penalty), np.float32(frequency_penalty), np.float32(penalty_decay)
        self.penalties: dict[int, np.float32] = {}
        self.bias = dict(bias or {})

    def init(self, model_tokens):                                    # nucleus.rs:49-59
        for index, token in enumerate(reversed(list(model_tokens))):
            pen = self.penalties.pop(int(token), self.ap)
            self.penalties[int(token)] = np.float32(pen + self.af * self.ad ** np.float32(index))

    def adjustments(self) -> dict:                                    # transform (nucleus.rs:61-67) + bias (run.rs:681-683)
        adj = {t: np.float32(-p) for t, p in self.penalties.items()}
        for t, b in self.bias.items():
            adj[t] = np.float32(adj.get(t, np.float32(0)) + np.float32(b))
        return adj

    def update(self, token: int):                                     # nucleus.rs:104-119
        for t in self.penalties:
            self.penalties[t] = np.float32(self.penalties[t] * self.ad)
        self.penalties[token] = np.float32(self.penalties[token] + self.af) if token in self.penalties else self.ap


class TypicalSampler(NucleusSampler):
    """Host-side state of `TypicalSampler` (sampler/typical.rs:11-140): the same penalty state machine as the nucleus
    sampler (init typical.rs:47-58, transform :62-68, update :122-133); the device applies tau / top_k / temperature."""
    kind = 1

    def __init__(self, tau=0.5, top_k=128, temperature=1.0, presence_penalty=0.3, frequency_penalty=0.3,
                 penalty_decay=0.99654026, bias: dict | None = None):
        super().__init__(top_p=0.0, top_k=top_k, temperature=temperature, presence_penalty=presence_penalty,
                         frequency_penalty=frequency_penalty, penalty_decay=penalty_decay, bias=bias)
        self.tau = float(tau)


class MirostatSampler:
    """Host-side state of `MirostatSampler` (sampler/mirostat.rs:11-90): `max_surprise` lives here; the device sorts,
    truncates at max_surprise, samples and returns the token surprise; `update()` applies mirostat.rs:85-87."""
    kind = 2
    top_k, temperature, top_p = 1, 1.0, 0.0

    def __init__(self, tau=3.0, rate=0.1):
        self.target, self.rate = np.float32(tau), np.float32(rate)
        self.max_surprise = np.float32(2.0 * tau)

    @property
    def tau(self):                                                    # what the device calls tau for kind 2
        return float(self.max_surprise)

    def init(self, model_tokens):                                     # mirostat.rs:38
        pass

    def adjustments(self) -> dict:                                    # transform is a no-op (mirostat.rs:40)
        return {}

    def update(self, token_surprise: float):
        err = np.float32(np.float32(token_surprise) - self.target)
        self.max_surprise = np.float32(min(np.float32(self.max_surprise - self.rate * err), np.float32(4.0) * self.target))


class DfaFormatter:
    """The reference's `Formatter` trait (sampler/bnf.rs:34-48) over a byte-level DFA (`runtime.Dfa`) — the host half of what
    `Runtime.gen_set_constraint` runs on the device, for the per-token path: `transform(mask)` is the mask `infer_sample` takes as `allow`
    (run.rs:676-679), `update(token) -> halt` advances and says whether the request stops (run.rs:892-897, 990).  A REGULAR constraint;
    the reference's kbnf (context-free) is another implementation of the same trait.

    `table[i]` is the bytes of token i, None for an unknown id (`gen_set_token_bytes`' table).  A token that is not allowed — id 0, an
    empty or unknown token, one whose bytes kill the walk — leaves the state where it was and does not halt (bnf.rs:44)."""

    def __init__(self, dfa, table, num_vocab: int, state: int | None = None, halt: int = 0):
        self.dfa, self.table, self.num_vocab, self.halt = dfa, list(table), int(num_vocab), int(halt)
        self.trans, self.accepting = dfa.table()
        self.state = dfa.start if state is None else int(state)

    def walk(self, state: int, word) -> int:
        if not word:
            return 0
        for c in word:
            state = int(self.trans[state, c])
            if not state:
                break
        return state

    def transform(self, mask=None):
        """the allowed-token mask of the current state, written into `mask` (uint8 [num_vocab]) when one is given"""
        allow = self.dfa.allow(self.state, self.table, self.num_vocab)
        if mask is not None:
            mask[:] = allow
            return mask
        return allow

    def update(self, token: int) -> bool:
        end = self.walk(self.state, self.table[token] if 0 < token < len(self.table) else None)      # token 0 is never allowed
        if not end:
            return False
        self.state = end
        if not self.accepting[end]:
            return False
        return self.halt == 1 or not self.trans[end].any()


class PdaFormatter:
    """The `Formatter` trait over a byte automaton with a return-state stack (`runtime.Pda`) — the host half of what `Runtime.gen_set_pda`
    runs on the device, for the per-token path: `transform()` is the `allow` mask of the configuration (rwkv_pda_allow), `update(token) ->
    halt` commits the token and says whether the request stops.  A token that is not allowed leaves the configuration where it was and
    does not halt; the mask decides what is allowed, so the span rule holds here as on the device."""

    def __init__(self, pda, table, num_vocab: int, state: int | None = None, stack=(), halt: int = 0):
        self.pda, self.table, self.num_vocab, self.halt = pda, list(table), int(num_vocab), int(halt)
        self.next, self.act, self.accepting = pda.table()
        self.state, self.stack = pda.start if state is None else int(state), [int(x) for x in stack]

    def transform(self, mask=None):
        allow = self.pda.allow(self.state, self.stack, self.table, self.num_vocab)
        if mask is not None:
            mask[:] = allow
            return mask
        return allow

    def update(self, token: int) -> bool:
        if not 0 < token < self.num_vocab or not self.transform()[token]:
            return False
        self.state, self.stack = self.pda.walk(self.table[token], self.state, self.stack)
        if self.stack or not self.accepting[self.state]:
            return False
        row_n, row_a = self.next[self.state], self.act[self.state]
        return self.halt == 1 or not ((row_a != 0xFFFF) & (row_n != 0)).any()


class StopMatcher:
    """The stop-STRING state machine of `process` (run.rs:855-869, 899-932, 990-1011), per token — the reference the device matcher
    (rwkv_gen_set_stops) is held to, and what a caller runs over the tokens it samples itself.

    Per token: the token's bytes join the buffer; every stop string walks the WHOLE buffer (on a mismatch `index_safe` moves behind the
    mismatching byte, which is not retried as a new start: "ab" over "aab" does not match); `min_by` picks a matched string before an
    unmatched one, then the smallest index, the first of equals; buffer = head | tail there.  A request that goes on sends the head and
    keeps the tail only if the head is valid UTF-8, else it keeps the whole buffer.  `cap` (the device's RWKV_GEN_STOP_BUF; None = no
    limit) bounds the buffer as the device's is bounded: a token that does not fit is not taken in and finishes with Handback."""
    RUNNING, STOP, LENGTH, HANDBACK = 0, 1, 2, 3                      # runtime.GenFinish

    def __init__(self, stops, tail: bytes = b"", cap: int | None = None):
        self.stops = [bytes(s) for s in stops]
        self.buffer = bytes(tail)
        self.cap = cap

    @staticmethod
    def scan(buffer: bytes, stop: bytes):                             # run.rs:905-924
        index_safe = index_unsafe = 0
        while index_unsafe < len(buffer):
            index_stop = index_unsafe - index_safe
            if index_stop >= len(stop):
                return index_safe, True
            differ = buffer[index_unsafe] != stop[index_stop]
            index_unsafe += 1
            if differ:
                index_safe = index_unsafe
        return index_safe, index_unsafe - index_safe >= len(stop)

    def split(self, buffer: bytes):
        """(mid, matched) of run.rs:900-932: `min` keeps the first minimum like Iterator::min_by; no stops: everything is head"""
        if not self.stops:
            return len(buffer), False
        return min((self.scan(buffer, s) for s in self.stops), key=lambda r: (not r[1], r[0]))

    def advance(self, word, stop_token: bool = False, at_max: bool = False):
        """One drawn token in the device's order (csrc/gen_stop.h gen_stop_decide).  `word` is the token's bytes, None for an id the
        tokenizer does not know (decode error: empty word and stop); `stop_token`: the token is 0 or a listed stop token; `at_max`: the
        request has `max_tokens` tokens with this one.  Returns (finish, content): the `Token::Content` bytes this token releases (on a stop
        the reference sends them through from_utf8_lossy).  A token that finishes leaves `tail()` as it was before it."""
        stop_token = stop_token or word is None
        grown = self.buffer + (word or b"")
        mid, matched = self.split(grown)
        if stop_token:
            return self.STOP, grown[:mid]
        if self.cap is not None and len(grown) > self.cap:
            return self.HANDBACK, b""
        if matched:
            return self.STOP, grown[:mid]
        if at_max:
            return self.LENGTH, b""
        try:
            grown[:mid].decode("utf-8")                               # String::from_utf8, run.rs:1008
        except UnicodeDecodeError:
            self.buffer = grown
            return self.RUNNING, b""
        self.buffer = grown[mid:]
        return self.RUNNING, grown[:mid]

    def push(self, word):
        """`word` (bytes, or None for a decode error) -> (stop_matched, content bytes to emit)"""
        fin, content = self.advance(word)
        self.handback = fin == self.HANDBACK
        return fin == self.STOP, content

    def tail(self) -> bytes:
        """what rwkv_gen_set_stops takes as `tail`: the bytes held back so far"""
        return self.buffer

    def replay(self, words):
        """The `Token::Content` pieces of a run's tokens (their bytes, None = unknown id), for a caller that got the tokens back from
        `gen_run`; stops behind the token that stops.  Returns (pieces, finish)."""
        pieces = []
        for w in words:
            fin, content = self.advance(w)
            pieces.append(content)
            if fin:
                return pieces, fin
        return pieces, self.RUNNING


class StateJob:
    """`GenerateKind::State` requests as a batch job with SLOT TURNOVER — the documented `/embeddings` route (docs/doc-api/openai.md:
    376-437; `GenerateKind::State` run.rs:980-989; `api/oai/state.rs:29-40`) fed a list of documents.  The scheduling is the reference's
    (`queue` run.rs:488-626 -> `infer` steps run.rs:1121-1157 -> `finish`), the C++ form is `rwkv::Scheduler::queue / step / state`
    (include/rwkv_scheduler.hpp): every idle slot takes the next waiting document (an `Empty` slot: nothing cached matches a fresh document, so
    the state it starts from is the initial one, written from a device-resident snapshot like `state.write(backed.clone(), batch)`
    run.rs:1104), all busy slots ride the same `infer` call (`RWKV_OPTION_NONE`: state-only, no head GEMM), and a slot whose document has
    been consumed hands over its embedding — one layer's WKV rows, `rwkv_state_back_layer_async` into pinned memory on the engine's copy
    stream — and is free for the next document at once: the read-back of a finished document overlaps the prefill of the following ones.

    `run(docs)` returns (embeddings [n_docs, N, C] in pinned memory, number of infer calls)."""

    def __init__(self, runtime, layer: int | None = None, arena=None):
        from .runtime import PinnedArena
        self.rt = runtime
        self.layer = runtime.info.num_layer - 1 if layer is None else int(layer)
        self._Arena = arena or PinnedArena           # `arena(shape)` -> object with `.array`, `.close()` (tests pass a numpy one)
        # the initial state, device-resident (state.init() -> load -> read once; `backed.clone()` afterwards)
        runtime.state.load(runtime.state.init(), 0)
        self.zero = runtime.state.read(0)
        self.out = None

    def run(self, docs: list):
        rt, B = self.rt, self.rt.max_batch
        N, Cn = getattr(rt.state, "layer_rows", rt.info.head_size), rt.info.num_emb    # rows a layer owns (V4: 3, not head_size)
        if self.out is None or self.out.array.shape[0] < len(docs):
            if self.out is not None:
                self.out.close()
            self.out = self._Arena((len(docs), N, Cn))
        out = self.out.array
        # documents as uint32 arrays, once: a step then hands the engine views (no per-token Python work per call); empty prompt => [0] (run.rs:489-492)
        arr = [np.asarray(d if len(d) else [0], dtype=np.uint32) for d in docs]
        waiting = deque(range(len(docs)))
        owner = [-1] * B                        # document id a slot works on
        none = np.zeros(0, np.uint32)
        rest = [none for _ in range(B)]         # its tokens not yet consumed
        calls = 0
        while waiting or any(o >= 0 for o in owner):
            for b in range(B):                  # `queue`: the next document takes an idle slot
                if owner[b] < 0 and waiting:
                    d = waiting.popleft()
                    rt.state.write(self.zero, b)
                    owner[b], rest[b] = d, arr[d]
            inp = RnnInput([RnnInputBatch(rest[b] if owner[b] >= 0 else none, RnnOption.NoOutput) for b in range(B)])
            inp, _ = rt.infer(inp)              # one step over <= token_chunk_size tokens of all busy slots
            calls += 1
            for b in range(B):
                if owner[b] < 0:
                    continue
                rest[b] = inp.batches[b].tokens
                if not len(rest[b]):            # `finish`: the embedding leaves on the copy stream, the slot is idle again
                    rt.state.embed_async(self.layer, b, out[owner[b]])
                    owner[b] = -1
        rt.state.sync()
        return out[:len(docs)], calls

    def close(self):
        if self.out is not None:
            self.out.close()
            self.out = None


class ReplicaRouter:
    """Request-level sharding over independent engines (one per GPU): round-robin for batch jobs, least-busy for
    interactive requests.  No collective: each replica owns its weights, slots and stream.  (The full policy —
    longest cached prefix first, full replicas skipped, one driving thread per engine — is the C++ `rwkv::ReplicaRouter`,
    include/rwkv_router.hpp; this class is the single-threaded form the Python tests drive.)"""

    def __init__(self, runtimes: list):
        self.loops = [InferLoop(r) for r in runtimes]
        self.busy = [0] * len(runtimes)

    def pick(self) -> int:
        """Least-busy replica that still has a free slot (ties: lowest index); -1 when every replica is full."""
        free = [j for j in range(len(self.busy)) if self.busy[j] < self.loops[j].rt.max_batch]
        if not free:
            return -1
        i = min(free, key=lambda j: self.busy[j])
        self.busy[i] += 1
        return i

    def release(self, i: int):
        self.busy[i] -= 1

    def generate(self, prompts: list, n_new: int) -> list:
        """Interactive requests: each prompt goes to the least-busy replica (`pick`), takes the next free slot there, and is
        decoded greedily (`greedy_process`); a prompt that finds every replica full waits for the current wave to finish."""
        out = [None] * len(prompts)
        todo = list(range(len(prompts)))
        while todo:
            wave = []
            used = [0] * len(self.loops)
            while todo:
                r = self.pick()
                if r < 0:
                    break
                i = todo.pop(0)
                wave.append((i, r, used[r]))
                used[r] += 1
            for i, r, slot in wave:
                self.loops[r].rt.state.load(self.loops[r].rt.state.init(), slot)
                out[i] = greedy_process(self.loops[r], slot, list(prompts[i]), n_new)
                self.release(r)
        return out

    @staticmethod
    def shard(n_items: int, rank: int, world: int) -> range:
        """Indices of a batch job owned by `rank` (documents round-robin)."""
        return range(rank, n_items, world)

    def embed_documents(self, docs: list, layer: int) -> list:
        """`/embeddings`-style job: prefill each document, return one layer's WKV rows as its embedding."""
        out = [None] * len(docs)
        for r, loop in enumerate(self.loops):
            mine = list(self.shard(len(docs), r, len(self.loops)))
            B = loop.rt.max_batch
            for g in range(0, len(mine), B):
                group = mine[g:g + B]
                for slot, d in enumerate(group):
                    loop.rt.state.load(loop.rt.state.init(), slot)
                    loop.submit(InferRequest(slot, list(docs[d]), RnnOption.NoOutput))   # state-only: no head GEMM, no logits
                loop.run_pending()
                for slot, d in enumerate(group):
                    out[d] = loop.rt.state.embed(layer, slot)
        return out
