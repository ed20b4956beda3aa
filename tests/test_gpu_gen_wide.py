"""MI355X: resident generation at the widths a server runs it at — 8 to 72 decode rows, mixed steps of 99 and 128 rows — against the
lock-step reference of tests/test_gpu_gen_prompt.py (`lockstep()`: a second engine of the same model driven per token by `infer_sample`
with the host samplers and `gen_uniform`, issued with the rows every resident step carries).  Nothing is compared with a tolerance: token
ids, the bits of `out_probs`, `n_emitted`, `finish`, and `state.back` of EVERY slot after EVERY run.

Engines have max_batch 72 and token_chunk_size 128.  The GEMM plan changes at 16|17, 32|33 and 64|65 rows; the width walk puts a decode
stretch on both sides of each, with row sets that have gaps, reach into the second word of the slot mask (slots 64 .. 71) and need every
sampler kernel.  A row set is new in every run, so its three steps are one direct step, the capture, and two replays of the captured
graph (`gen_decode_steps`)."""
import copy

import numpy as np
import pytest

from ai00_server_amd import runtime as rt
from oracle import rwkv_ref as R
from tests import test_gpu_gen_prompt as GP
from tests import test_gpu_generate as GG

pytestmark = pytest.mark.gpu

PAD, SEED = GP.PAD, GP.SEED
B, CHUNK, RUN = 72, 128, 3
MODELS = [("v6-small", (3, 1)), ("v7-small", (3, 2)), ("v5-small", (2, 1))]
KINDS = ("nucleus", "typical", "mirostat")
WIDTHS = [72, 65, 64, 33, 32, 17, 16, 9, 8]                        # live slots per run: both sides of 64|65, 32|33 and 16|17
GROUPS = [(3, 7), (6, 1), (9, 31), (12, 1), (15, 15), (18, 1), (21, 7), (24, 1), (27, 8)]   # (max_tokens, slots)
TAIL = [0, 63, 64, 71]                                             # among the eight that run to the end: both ends of both mask words
ORDER = [b for b in sorted(range(B), key=lambda b: b * 29 % B) if b not in TAIL] + TAIL
MAXTOK = {}
for _n, _at in zip([n for n, c in GROUPS for _ in range(c)], ORDER):
    MAXTOK[_at] = _n
STOP_GROUPS = (3, 9, 15, 21)                                       # the groups that end in runs 1, 3, 5 and 7: two slots of each stop one step early
BASES = (200, 300, 400, 500, 600, 700)                             # prompt seeds, tried in turn until no slot draws token 0 (which ends a slot)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_the_schedule_is_the_one_the_widths_need():
    assert sorted(ORDER) == list(range(B)) and sum(c for _, c in GROUPS) == B and all(n % RUN == 0 for n, _ in GROUPS)
    assert [sum(MAXTOK[b] >= RUN * (r + 1) for b in range(B)) for r in range(9)] == WIDTHS
    last = [b for b in range(B) if MAXTOK[b] == 27]
    assert len(last) == 8 and set(TAIL) <= set(last)
    for r in range(9):                                             # every row set has gaps
        live = [b for b in range(B) if MAXTOK[b] >= RUN * (r + 1)]
        assert r == 0 or live != list(range(live[0], live[0] + len(live)))


def sampler_of(b, V):
    """kind b % 3; the three variants of test_gpu_generate.samplers (no presence penalty and a bias that makes repeats certain | defaults and
    a bias | defaults) in turn"""
    return GG.samplers(KINDS[b % 3], V)[b // 3 % 3]


def reset(eng):
    init = eng.state.init()
    for b in range(eng.max_batch):
        eng.state.load(init, b)


def prepare(eng, base, slots):
    """prompts of 3 + b % 5 tokens consumed on `slots` of a zeroed engine; (prompts, first tokens, samplers as gen_arm takes them)"""
    V = eng.info.num_vocab
    reset(eng)
    prompts = [GG.prompt(V, base + b, 3 + b % 5) if b in slots else [] for b in range(B)]
    first = GG.prefill(eng, prompts)
    smp = {}
    for b in slots:
        smp[b] = sampler_of(b, V)
        smp[b].init(prompts[b])
        if not GP.is_miro(smp[b]):
            smp[b].update(first[b])
    return prompts, first, smp


def compare(A, got, T, P, fins, states, what):
    """one gen_run against one lockstep call, every slot of the engine"""
    t, p, ne, fin = got
    for b in range(B):
        on = T[:, b] != PAD
        assert (t[:, b] == T[:, b]).all(), (what, "slot", b, "want", T[:, b].tolist(), "got", t[:, b].tolist())
        assert np.isnan(p[~on, b]).all() and (bits(p[on, b]) == bits(P[on, b])).all(), (what, "slot", b, "probs")
        assert int(ne[b]) == int(on.sum()) and int(fin[b]) == fins.get(b, 0), (what, "slot", b, int(ne[b]), int(fin[b]), fins.get(b, 0))
        if b in states:
            assert (bits(A.state.back(b)) == bits(states[b])).all(), (what, "slot", b, "state")


def walk(Bn, slabs, first, smp, stops):
    """the nine runs of the width walk on the reference engine, from the prefilled states `slabs`"""
    for b, s in slabs.items():
        Bn.state.load(s, b)
    jobs = {b: GP.Job([first[b]], copy.deepcopy(smp[b]), MAXTOK[b], b, False, stops.get(b, ())) for b in range(B)}
    runs = []
    for _ in WIDTHS:
        live = sum(not j.fin_seen for j in jobs.values())
        rows = []
        T, P = GP.lockstep(Bn, jobs, RUN, rows=rows)
        runs.append(dict(live=live, rows=rows, T=T, P=P, fins={b: j.fin for b, j in jobs.items()}, states={b: j.state for b, j in jobs.items()}))
    return jobs, runs


@pytest.mark.parametrize("name,quant", MODELS)
def test_width_walk_72_to_8_rows(name, quant):
    A, Bn = GP.build_pair(name, B, quant, chunk=CHUNK)
    V = A.info.num_vocab
    for base in BASES:
        prompts, first, smp = prepare(Bn, base, range(B))
        slabs = {b: Bn.state.back(b) for b in range(B)}
        # the reference without stops: which token each slot emits at the second draw of its last run
        dry, _ = walk(Bn, slabs, first, smp, {})
        toks = {b: [x for x, _ in dry[b].out] for b in range(B)}
        stops = {}
        for n in STOP_GROUPS:
            ok = [b for b in ORDER if MAXTOK[b] == n and toks[b][n - 2:n - 1] and toks[b][n - 2] not in toks[b][:n - 2]][:2]
            stops.update({b: [toks[b][n - 2]] for b in ok})
        if all(len(toks[b]) == MAXTOK[b] and 0 not in toks[b] for b in range(B)) and len(stops) == 2 * len(STOP_GROUPS):
            break
        print(name, "prompts", base, "draw token 0 or leave no stop candidates: next prompts")
    else:
        raise AssertionError("no prompt set keeps the width schedule: extend BASES")
    jobs, runs = walk(Bn, slabs, first, smp, stops)
    print(name, "prompts", base, "live", [r["live"] for r in runs], "rows per step", [[x for x, _ in r["rows"]] for r in runs])
    print(name, "stop slots", {b: (MAXTOK[b], s[0]) for b, s in stops.items()})
    assert [r["live"] for r in runs] == WIDTHS
    assert [[x for x, _ in r["rows"]] for r in runs] == [[w] * RUN for w in WIDTHS]
    for b in range(B):                                             # a stop slot finishes one step early, with Stop, and rides the third step
        want = (MAXTOK[b] - 1, int(rt.GenFinish.Stop)) if b in stops else (MAXTOK[b], int(rt.GenFinish.Length))
        assert (len(jobs[b].out), jobs[b].fin) == want, (b, len(jobs[b].out), jobs[b].fin)
    assert {b % 3 for b in range(B) if MAXTOK[b] == 27} == {0, 1, 2}   # the narrowest row set still needs every sampler kernel
    assert GG.prefill(A, prompts) == first
    for b in range(B):
        A.gen_arm(b, first[b], MAXTOK[b], copy.deepcopy(smp[b]), seed=SEED, stop_tokens=stops.get(b, ()))
    for r, ref in enumerate(runs):
        compare(A, A.gen_run(RUN), ref["T"], ref["P"], ref["fins"], ref["states"], (name, "run", r, "width", ref["live"]))
    t, _, ne, _ = A.gen_run(RUN)                                    # everything finished: nothing moves
    assert (t == PAD).all() and not ne.any()
    A.close()
    Bn.close()


# ---- admission at width ------------------------------------------------------------------------------------------------------------------
DEC = sorted(5 * i % B for i in range(40))                         # 40 scattered decode slots, 63, 65, 68 and 70 among them
ADMIT = {64: (1, "nucleus", 2), 2: (30, "typical", 2), 71: (200, "mirostat", 5)}   # slot: (prompt length, sampler, max_tokens)
ITEM, ITEM_MAX, ITEM_PROMPT = 37, 2, 11
MIXED = [(128, 40), (128, 43), (99, 40)]                           # (rows, decode rows among them) of the three mixed steps


def test_admission_at_width():
    """40 slots decode (three steps at 40 rows); then three prompts of 1, 30 and 200 tokens and a slot armed from an item are admitted
    between two runs.  The first mixed step carries 127 step rows and the item's row: 40 decode rows, the two short prompts whole and 56
    rows of the long one.  The second carries the 43 decode rows there are now and 85 rows of the long prompt.  The two short prompts and
    the item slot have max_tokens 2 and are gone by the third, which carries 40 decode rows and the last 59 of the long prompt.  Then 41
    slots decode; the long prompt's slot finishes two steps before the run ends and rides.
    The item slot's first (token, prob) are those of the same request armed with its prompt on an engine of one slot — a row's draw does
    not depend on its neighbours — and from its second draw on it is a Job of the lock-step reference like the others."""
    name, quant = MODELS[0]
    Cap = rt.GenCapture
    A, Bn = GP.build_pair(name, B, quant, chunk=CHUNK)
    E = rt.ModelBuilder(R.st_serialize(R.synth_named(name))).quant(quant[0], rt.Quant(quant[1])).build(max_batch=1, token_chunk_size=CHUNK, precision=rt.Precision.Fp16)
    V = A.info.num_vocab
    assert not set(DEC) & (set(ADMIT) | {ITEM}) and max(DEC) >= 64 and len(DEC) == 40
    # the item: captured behind its prompt on the one-slot engine, moved through the host
    ip = GG.prompt(V, 900, ITEM_PROMPT)
    ismp = GP.make_sampler("nucleus")
    ismp.init(ip)
    E.gen_arm_prompt(0, ip, 1, copy.deepcopy(ismp), seed=SEED, stream=ITEM)
    E.gen_set_capture(0, Cap.Prompt)
    t, p, ne, fin = E.gen_run(2)
    assert int(ne[0]) == 1 and t[0, 0] != PAD and t[0, 0] != 0, "the item's first token is token 0: pick another prompt"
    tok0, prob0 = int(t[0, 0]), p[0, 0]
    ist, irow = E.gen_take_item(0, Cap.Prompt).back()
    E.close()
    for base in BASES:
        prompts, first, smp = prepare(Bn, base, DEC)
        jobs = {b: GP.Job([first[b]], copy.deepcopy(smp[b]), 12, b, False) for b in DEC}
        rows1, rows2 = [], []
        T1, P1 = GP.lockstep(Bn, jobs, RUN, rows=rows1)
        ref1 = dict(fins={b: j.fin for b, j in jobs.items()}, states={b: j.state for b, j in jobs.items()})
        admit = {}
        for b, (n, kind, mx) in ADMIT.items():
            q = GG.prompt(V, base + 100 + b, n)
            s = GP.make_sampler(kind)
            s.init(q)
            admit[b] = (q, s, mx)
            jobs[b] = GP.Job(q, copy.deepcopy(s), mx, b, True)
        Bn.state.load(ist, ITEM)
        s = copy.deepcopy(ismp)
        s.update(tok0)
        jobs[ITEM] = GP.Job([tok0], s, ITEM_MAX, ITEM, False, draws=1, emitted=[(tok0, prob0)])
        T2, P2 = GP.lockstep(Bn, jobs, 9, pseudo=[ITEM], rows=rows2)
        T2[0, ITEM], P2[0, ITEM] = tok0, prob0                        # the draw from the item's row, made in the first step
        if all(j.fin == int(rt.GenFinish.Length) and len(j.out) == j.n for j in jobs.values()):
            break
        print("prompts", base, "draw token 0: next prompts")
    else:
        raise AssertionError("every prompt set draws token 0: extend BASES")
    print("prompts", base, "rows of run 1", rows1, "rows of run 2", rows2)
    assert rows1 == [(40, 40)] * RUN
    assert rows2[:3] == MIXED and rows2[3:] == [(41, 41)] * 6
    assert len(jobs[71].out) == 5 and (T2[7:, 71] == PAD).all() and T2[6, 71] != PAD   # the long prompt's slot rides the last two steps
    # the resident side
    assert GG.prefill(A, prompts) == first
    for b in DEC:
        A.gen_arm(b, first[b], 12, copy.deepcopy(smp[b]), seed=SEED)
    compare(A, A.gen_run(RUN), T1, P1, ref1["fins"], ref1["states"], "run 1")
    for b, (q, s, mx) in admit.items():
        A.gen_arm_prompt(b, q, mx, copy.deepcopy(s), seed=SEED)
    item = rt.GenItem.from_host(A, ist, irow)
    A.gen_arm_item(ITEM, item, ITEM_MAX, copy.deepcopy(ismp), seed=SEED, stream=ITEM)
    compare(A, A.gen_run(9), T2, P2, {b: j.fin for b, j in jobs.items()}, {b: j.state for b, j in jobs.items()}, "run 2")
    item.close()
    A.close()
    Bn.close()
