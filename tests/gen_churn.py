"""The visit list that drives `gen_graphs` — the 64-entry cache of captured decode steps in `gen_decode_steps` (rwkv_engine.cpp) — past its
capacity, shared by tests/test_gpu_gen_churn.py (runs it on the GPU against the lock-step reference) and tests/test_gen_churn_cpu.py (replays
its keys through the real rwkv::GraphCache and proves that the schedule evicts, captures again and replays).

An engine of 72 slots, seven seats.  A visit arms exactly the seats of its row set with max_tokens 3 and runs three steps, so every visit is
one decode-only stretch on one key.  The key, as `gen_decode_steps` forms it: the slot mask in (max_batch + 63) / 64 words, then a flag word
— the sampler kernels the rows need in its low bits, and one bit each for stop strings (32), a byte automaton (33), top-n lists (34), a
stack automaton (35), an open watch (36) and FINISH capture (37)."""
import itertools

MAX_BATCH = 72
SEATS = (0, 1, 31, 63, 64, 65, 71)                                 # both ends of both mask words
KINDS = ("nucleus", "typical", "mirostat")                        # seat i samples with KINDS[i % 3]
NEEDS_NT, NEEDS_MIRO = 1, 2                                        # rwkv_engine.cpp: nucleus / typical rows, Mirostat rows
STOPS, TOPN, WATCH = 1 << 32, 1 << 34, 1 << 36
CAPACITY = 64

SETS = list(itertools.combinations(range(len(SEATS)), 3)) + list(itertools.combinations(range(len(SEATS)), 4))   # 35 + 35 distinct row sets
VISITS = SETS + SETS[:3] + SETS[-3:]                               # ... then the three oldest again (evicted by then) and the three newest (still cached)
BANDS = {"watch": range(20, 30), "topn": range(30, 40), "stops": range(40, 50)}
TOPN_N = 4
STOP_STRING = b"zz"                                                # over a byte no token of the table produces (test_gpu_gen_stop.table: a, b, c and pieces of UTF-8)


def band(visit):
    return next((name for name, r in BANDS.items() if visit in r), None)


def featured(visit):
    """the seat (an index into SEATS) that lists or carries the stop string in a visit of those bands: the first of the row set"""
    return VISITS[visit][0]


def stream(visit, seat):
    return visit * 8 + seat


def key(visit):
    words = [0] * ((MAX_BATCH + 63) // 64)
    needs = 0
    for i in VISITS[visit]:
        words[SEATS[i] // 64] |= 1 << (SEATS[i] % 64)
        needs |= NEEDS_MIRO if KINDS[i % 3] == "mirostat" else NEEDS_NT
    return tuple(words) + (needs | {"watch": WATCH, "topn": TOPN, "stops": STOPS, None: 0}[band(visit)],)


def keys():
    return [key(v) for v in range(len(VISITS))]
