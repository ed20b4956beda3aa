"""The reference's per-token stop logic, transcribed LITERALLY (crates/ai00-core/src/run.rs:855-869, 899-932, 990-1011) with
`bytes.decode("utf-8")` standing for `String::from_utf8`, and its trace in the device's terms.  Shared by tests/test_gen_stop_cpu.py (which
holds the host matchers and gen_stop.h to it) and tests/gen_cases.py (which holds gen_post_kernel<., true> to it).  A plain module, no fixtures."""
import functools

CAP = 512                                                          # RWKV_GEN_STOP_BUF


def ref_scan(buffer: bytes, stop: bytes):
    """run.rs:905-924"""
    index_safe = 0
    index_unsafe = 0
    while index_unsafe < len(buffer):
        index_stop = index_unsafe - index_safe
        if index_stop >= len(stop):
            return (index_safe, True)
        output = buffer[index_unsafe]
        st = stop[index_stop]
        index_unsafe += 1
        if output != st:
            index_safe = index_unsafe
    return (index_safe, index_unsafe - index_safe >= len(stop))


def ref_min_by(x, y):
    """run.rs:926-930"""
    if (x[1], y[1]) == (True, False):
        return -1
    if (x[1], y[1]) == (False, True):
        return 1
    return (x[0] > y[0]) - (x[0] < y[0])


def ref_process(stops, tokens, max_tokens, tail=b"", emitted=0):
    """`tokens`: [(token id, bytes or None when `tokenizer.decode` fails)].  Yields per token (decision, head, buffer afterwards) with
    decision in Stop / Length / Content (head sent, buffer = tail) / Hold (head is not UTF-8: nothing sent, buffer kept whole)."""
    buffer = bytes(tail)
    n_model_tokens = emitted
    for token, word in tokens:
        stop_token = token == 0                                          # run.rs:855
        if word is None:                                                 # run.rs:858-862
            stop_token = True
            word = b""
        n_model_tokens += 1                                              # run.rs:867
        buffer = buffer + word                                           # run.rs:869
        results = [ref_scan(buffer, s) for s in stops]
        if results:
            mid, stop_matched = min(results, key=functools.cmp_to_key(ref_min_by))    # min, like Iterator::min_by, keeps the first of equals
            head, tl = buffer[:mid], buffer[mid:]
        else:
            (head, tl), stop_matched = (buffer, b""), False              # run.rs:932
        if stop_matched or stop_token:                                   # run.rs:990
            yield "Stop", head, buffer
            return
        elif n_model_tokens >= max_tokens:                               # run.rs:1006
            yield "Length", head, buffer
            return
        else:
            try:
                head.decode("utf-8")                                     # run.rs:1008
            except UnicodeDecodeError:
                yield "Hold", b"", buffer
                continue
            buffer = tl                                                  # run.rs:1010
            yield "Content", head, buffer


def expected(stops, tokens, max_tokens, tail=b"", emitted=0):
    """The reference's trace in the device's terms: [(finish, content, buffer afterwards)], with the bounded buffer put in — a token whose
    bytes would take the buffer past CAP, and that is no stop token, is RWKV_GEN_HANDBACK.  A token that finishes leaves the buffer as it
    was before it (the reference drops the request's buffer then; the device documents this)."""
    out, buffer = [], bytes(tail)
    for (token, word), (dec, head, after) in zip(tokens, ref_process(stops, tokens, max_tokens, tail, emitted)):
        stop_token = token == 0 or word is None
        over = len(buffer) + len(word or b"") > CAP
        if over and not stop_token:
            out.append((3, b"", buffer))
            return out
        if dec == "Stop":
            out.append((1, None if over else head, buffer))              # a stop TOKEN that does not fit: the head is not compared
            return out
        if dec == "Length":
            out.append((2, b"", buffer))
            return out
        buffer = after
        out.append((0, head, buffer))
    return out
