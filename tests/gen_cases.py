"""The resident-generation probe's case table and references, shared by tests/test_gpu_gen_exact.py (runs tests/cpp/gen_probe.hip on the GPU)
and tests/test_gen_cases_cpu.py (proves table, references and checker without a GPU): one launch of one gen_* launcher per case (DESIGN.md
"Resident-generation probe").

A case is a WORLD: role -> array, one role per member of GenArgs plus the memory roles nested pointers point into.  Every buffer has a
256-element guard band on both sides, the logits block a spare row on both sides, and EVERY buffer is copied back whole.  The reference of a
launcher (`REF`) rewrites a copy of the world in place, in Python, from the kernels' comments and the host headers' contracts and without
calling either; `check_case` then compares every buffer with the expected world bit for bit, guard bands and spare rows included.  The
exceptions, all of them: the places gen_topn's ln-probabilities and ln S go (the bound of tests/topn_cases.py); a cell in which the launch
computes a NaN from a penalty entry that is a NaN (it must hold a NaN, and in a penalty row still an entry: the payload is the hardware's);
and the penalty row of a slot whose `finish` was non-zero on entry to gen_post (dead data by the kernel's own comment; the reference does
not model it).

Structures travel as numpy structured arrays of the C layouts (the probe asserts the sizes); a nested pointer is an int64 offset into its
memory role, -1 for null, and comes back as 0 (gen_probe.hip's header states the rule)."""
import copy
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests import topn_cases as TN
from tests.probe_io import GUARD, SENT, SENT32, UINT, Buf, own, read_results, untouched   # noqa: F401  (the container: stated once, there)
from tests.probe_io import write_cases as write_case_file
from tests.stop_ref import expected as stop_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, U32, I32, U16, U8 = np.float32, np.float64, np.uint32, np.int32, np.uint16, np.uint8
INF = np.inf
MAGIC = 0x4E454750
ABSENT = 0xFFFFFFFF                                                # GEN_ABSENT
TOK_UNKNOWN = 0x80000000                                           # GEN_TOK_UNKNOWN
NO_TOKEN = 0xFFFFFFFF                                              # GEN_WATCH_NO_TOKEN
POP = 0xFFFF                                                       # GEN_PDA_POP
SPAN, MAX_DEPTH, TOKEN_LEN, TOPN_MAX = 8, 64, 256, 32              # GEN_PDA_TOKEN_SPAN, GEN_PDA_MAX_DEPTH, GEN_TOKEN_LEN, TOPN_MAX
M64 = (1 << 64) - 1

KIND_NAME = ("gen_pre", "gen_topn", "gen_mask", "gen_post", "gen_publish", "gen_freeze", "gen_capture", "gen_inject", "gen_tokens", "gen_handover",
             "topn_pair", "gen_pda_mask", "step")
KIND = {n: i for i, n in enumerate(KIND_NAME)}
PARAMS = ("V", "max_batch", "n_rows", "T", "mixed", "n_tok", "steps", "nsx", "nw", "first_row", "to_held", "dfa_states", "ring_steps", "n",
          "pda_states", "n_steps", "any_miro", "cancel_step", "cancel_slot")
_ROLES = ("slots dfa tok_end tok_off tok_bytes row_slot out_rows held logits penalty bias rows samp_tok samp_prob feedback out_tok out_prob run_step sxa sxf wkv "
          "shadow topn_n top_ids top_logp tok_logp side_ms side_rows watch cap token dfa_trans dfa_flags cap_mem shadow_mem ring out_ids2 out_logp2 side_ms2 "
          "side_rows2 stops pda pda_next pda_act pda_flags logits_steps").split()
ROLE = {n: i for i, n in enumerate(_ROLES)}                        # the Role enum of gen_probe.hip
GROUPS = ("pre", "post", "stops", "mask", "pda", "topn", "state", "publish", "tokens", "step")
VOCABS = (16, 1024, 16384, 16400, 65536)                           # gen_pre, gen_post's penalty pass, gen_inject: 16 blocks x 256 threads x float4 = 16384 a pass
MASK_VOCABS = (16, 272, 65536)                                     # gen_mask, gen_pda_mask: min(ceil(V / 256), 256) blocks of 256 ids
SX_STRIDES, WKV_STRIDES = (64, 65600), (64, 131136)                # gen_freeze, gen_capture: 64 blocks x 256 x float4 = 65536 floats a pass
WIDE_B = 72                                                        # the wide worlds (geom): more rows than a wavefront has lanes, slot ids past 64
TOKEN_ROWS = (0, 1, 256, 257, 300)                                 # gen_tokens, gen_handover: ceil(T / 256) blocks of 256 rows

SLOT_DT = np.dtype([("top_p", "<f4"), ("top_k", "<i4"), ("temperature", "<f4"), ("tau", "<f4"), ("kind", "<i4"), ("presence", "<f4"), ("frequency", "<f4"),
                    ("decay", "<f4"), ("miro_target", "<f4"), ("miro_rate", "<f4"), ("seed", "<u8"), ("stream", "<u4"), ("draws", "<u4"), ("max_tokens", "<i4"),
                    ("emitted", "<i4"), ("finish", "<i4"), ("freeze_at", "<i4"), ("has_bias", "<i4"), ("n_stop", "<i4"), ("stop", "<u4", (8,)), ("wide", "<i4"),
                    ("pad", "<u4")])
STOP_DT = np.dtype([("str", "u1", (8, 128)), ("buf", "u1", (512,)), ("len", "<u2", (8,)), ("n_str", "<i4"), ("buf_len", "<i4"), ("pad", "<u4", (2,))])
DFA_DT = np.dtype([("trans", "<i8"), ("flags", "<i8"), ("state", "<i4"), ("mode", "<i4")])
PDA_DT = np.dtype([("stack", "<u2", (64,)), ("next", "<i8"), ("act", "<i8"), ("flags", "<i8"), ("state", "<i4"), ("depth", "<i4"), ("mode", "<i4"),
                   ("max_depth", "<i4"), ("pad", "<u4", (2,))])
CAP_DT = np.dtype([("p_state", "<i8"), ("p_row", "<i8"), ("f_row", "<i8"), ("inj_row", "<i8")])
WATCH_DT = np.dtype([("ring", "<i8"), ("cancel", "<i8"), ("seq", "<u8"), ("ring_steps", "<i4"), ("reserved", "<i4")])
SP_DT = np.dtype([("top_p", "<f4"), ("top_k", "<i4"), ("temperature", "<f4"), ("uniform", "<f4"), ("kind", "<i4"), ("tau", "<f4")])
assert (SLOT_DT.itemsize, STOP_DT.itemsize, DFA_DT.itemsize, PDA_DT.itemsize, CAP_DT.itemsize, WATCH_DT.itemsize, SP_DT.itemsize) == (120, 1568, 24, 176, 32, 32, 24)
POINTERS = {"dfa": ("trans", "flags"), "pda": ("next", "act", "flags"), "cap": ("p_state", "p_row", "f_row", "inj_row"), "watch": ("ring", "cancel")}
TOLERANT = ("top_logp", "side_ms", "out_logp2", "side_ms2")        # what gen_topn computes with logf / expf: held to topn_cases' bound, all else to the bit
MISTAKES = ("fused_decay", "assoc_left", "by_value", "by_isnan", "topn_at_run_step", "feedback_slot", "row_slot_mixed", "max_lt", "stack_stage_64", "span_9",
            "capture_rider", "freeze_always", "cancel_no_draw", "stamp_seq", "guard_write", "neighbour_penalty")


@dataclass
class Case:
    name: str
    group: str
    kind: int
    p: dict
    o: dict = field(default_factory=dict)                          # world: the function that makes the case's world; tags: what the case covers


# ------------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------------
def words(a):
    """The bits of a world array as the probe carries them: bytes for the 8- and 16-bit planes, 4-byte words for everything else."""
    a = np.ascontiguousarray(a)
    return a.view(U8 if a.dtype.names is None and a.dtype.itemsize < 4 else U32).reshape(-1)


def bufs_of(W, V):
    out = []
    for role in _ROLES:
        if role in W:
            b = words(W[role])
            spare = V if role == "logits" else 0
            s = SENT[b.dtype.itemsize]
            g, sp = np.full(GUARD, s, b.dtype), np.full(spare, s, b.dtype)
            if (b == s).all():                                     # nothing but the pattern: the probe fills it, the file carries no image
                out.append(Buf(role, b.dtype.itemsize, 3, b.size + 2 * spare, spare))
            else:
                out.append(Buf(role, b.dtype.itemsize, 1, b.size + 2 * spare, spare, np.concatenate([g, sp, b, sp, g])))
    assert {k for k in W if not k.startswith("_")} <= set(_ROLES), set(W) - set(_ROLES)
    return out


def image_of(b):
    return np.full(b.n + 2 * GUARD, SENT[b.esize], UINT[b.esize]) if b.flags & 2 else b.image


def write_cases(path, cases, datas):
    return write_case_file(path, MAGIC, cases, datas, lambda c: PARAMS, ROLE)


def plan_line(c):
    if KIND_NAME[c.kind] == "step":
        W = c.o["world"]()
        launches = (("tokens," if c.p["mixed"] else "") + ("inject," if "cap" in W and c.p["mixed"] and c.p["first_row"] < c.p["n_rows"] else "")
                    + ("capture," if "cap" in W else "") + ("topn," if "topn_n" in W else "") + "pre," + ("mask," if "dfa" in W else "") + ("pda_mask," if "pda" in W else "")
                    + "nucleus,post," + ("publish," if "watch" in W else "") + f"freeze x {c.p['n_steps']}")
        return {"case": c.name, "launches": launches, "launcher": "step", "mixed": int(c.p["mixed"]), "stops": 0, "n_rows": int(c.p["n_rows"]), "V": int(c.p["V"]),
                "max_batch": int(c.p["max_batch"])}
    return {"case": c.name, "launcher": KIND_NAME[c.kind], "mixed": int(c.p["mixed"]), "stops": int(c.group == "stops"), "n_rows": int(c.p["n_rows"]), "V": int(c.p["V"]),
            "max_batch": int(c.p["max_batch"])}


def build_probe():
    from ai00_server_amd import build as B
    return B.build_probe("gen_probe", verbose=False)


def make(c):
    W = c.o["world"]()
    return {"bufs": bufs_of(W, c.p["V"]), "W": W}


def sent(n):
    return np.full(int(n), SENT32, U32)


# ------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------
def uniform(seed, stream, step):
    """gen_uniform_draw: SplitMix64 of the counter (stream << 32 | step) + 1 behind the seed; the top 24 bits times 2^-24."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * ((((int(stream) << 32) | int(step)) + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return F32((z >> 40) * 2.0 ** -24)


def slot_of(W, p, row, bug=None):
    if p["mixed"] and bug != "row_slot_mixed":
        return int(W["row_slot"][W["out_rows"][row]])
    return int(W["row_slot"][row])


def adjust(x, pbits, b, bug=None):
    """gen_adjust over a row: x + ((-p) + b) where the slot has an entry, x + b where it has none; a zero bias adds nothing."""
    with np.errstate(invalid="ignore", over="ignore"):
        present = np.ones(x.size, bool) if bug == "by_value" else pbits != ABSENT
        if bug == "by_isnan":
            present = ~np.isnan(pbits.view(F32))
        neg = -pbits.view(F32)
        if bug == "assoc_left":
            with_p = np.where(b != 0, ((x + neg).astype(F32) + b).astype(F32), (x + neg).astype(F32))
        else:
            with_p = np.where(b != 0, (x + (neg + b).astype(F32)).astype(F32), (x + neg).astype(F32))
        without = np.where(b != 0, (x + b).astype(F32), x)
        return np.where(present, with_p, without).astype(F32)


def ref_pre(W, p, bug=None):
    if not p["mixed"]:
        W["run_step"][0] += 1
    rows = W["rows"].view(SP_DT)
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        g = W["slots"][slot]
        if g["finish"]:
            if p["mixed"]:
                rows[row] = (0.0, 0, 1.0, 0.0, 0, 0.0)
            continue
        rows[row] = (g["top_p"], g["top_k"], g["temperature"], uniform(g["seed"], g["stream"], g["draws"]), g["kind"] | g["wide"], g["tau"])
        pen = g["kind"] != 2
        if not pen and not g["has_bias"]:
            continue
        V = p["V"]
        pb = W["penalty"][slot].view(U32) if pen else np.full(V, ABSENT, U32)
        b = W["bias"][slot] if g["has_bias"] else np.zeros(V, F32)
        W["logits"][row] = adjust(W["logits"][row], pb, b, bug)
        if bug == "guard_write" and row == 0:
            W["_guard"] = ("logits", -1)
        if bug == "neighbour_penalty" and row == 0:
            W["penalty"][(slot + 1) % p["max_batch"], 0] = F32(1.0)


def decay_row(pbits, tok, decay, freq, pres, bug=None):
    """gen_decay over a row: every entry times decay; the drawn token's entry then takes + frequency, or becomes `presence` where it had none."""
    out = pbits.copy()
    present = ~np.isnan(pbits.view(F32)) if bug == "by_isnan" else pbits != ABSENT
    pf = pbits.view(F32)
    with np.errstate(invalid="ignore"):
        dec = (pf * decay).astype(F32)
    out[present] = dec.view(U32)[present]
    if 0 <= tok < pbits.size:
        if present[tok]:
            v = F32(F64(pf[tok]) * F64(decay) + F64(freq)) if bug == "fused_decay" else F32(dec[tok] + freq)
        else:
            v = F32(pres)
        out[tok] = np.array([v], F32).view(U32)[0]
    return out


def mirostat(max_surprise, surprise, target, rate):
    err = F32(F32(surprise) - F32(target))
    step = F32(F32(rate) * err)
    return F32(min(F32(F32(max_surprise) - step), F32(F32(4.0) * F32(target))))


def token_word(W, p, tok):
    """The bytes of id `tok` in the world's token table, or None: not in the table, or marked unknown."""
    if not 0 <= tok < p["n_tok"]:
        return None
    o0, o1 = int(W["tok_off"][tok]), int(W["tok_off"][tok + 1])
    if o0 & TOK_UNKNOWN:
        return None
    return bytes(W["tok_bytes"][o0:max(o0, o1 & ~TOK_UNKNOWN)][:TOKEN_LEN])


def dfa_ends(trans, q, off, byts, n_tok, V):
    """gen_dfa_token_end for every id of a row: the state the token's bytes lead to from q, 0 where the token is not allowed."""
    e = np.zeros(V, U16)
    if q == 0 or n_tok <= 0:
        return e
    o = off[:n_tok + 1].astype(np.int64)
    known = (o[:-1] & TOK_UNKNOWN) == 0
    beg, end = o[:-1] & ~TOK_UNKNOWN, o[1:] & ~TOK_UNKNOWN
    ln = np.clip(end - beg, 0, TOKEN_LEN)
    ok = known & (ln > 0)
    ok[0] = False
    ids = np.nonzero(ok)[0]
    st = np.full(ids.size, q, np.int64)
    for i in range(int(ln[ids].max()) if ids.size else 0):
        act = (i < ln[ids]) & (st != 0)
        st[act] = trans[st[act], byts[beg[ids][act] + i]]
    e[ids] = st
    return e


def ref_mask(W, p, bug=None):
    V = p["V"]
    ends = W["tok_end"].reshape(p["n_rows"], V)
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        d = W["dfa"][slot]
        if W["slots"][slot]["finish"] or d["trans"] == -1:
            continue
        trans = W["dfa_trans"][d["trans"] // 2:][:p["dfa_states"] * 256].reshape(-1, 256)
        e = dfa_ends(trans, int(d["state"]), W["tok_off"], W["tok_bytes"], p["n_tok"], V)
        ends[row] = e
        W["logits"][row][e == 0] = -INF


def pda_walk(nxt, act, max_depth, q, base, word, span=SPAN):
    """A token's bytes from (q, base) on a real list: the state (0: not allowed), the stack behind it, the lowest depth reached."""
    st = list(base)
    low = len(st)
    for b in word:
        if q == 0:
            break
        a, t = int(act[q][b]), int(nxt[q][b])
        if a == 0:
            q = t
        elif a == POP:
            if st:
                q = st.pop()
                low = min(low, len(st))
            else:
                q = 0
        elif t == 0 or len(st) >= max_depth or len(st) - low >= span:   # the span rule: a token owns at most 8 entries
            q = 0
        else:
            st.append(a)
            q = t
    return q, st, low


def pda_tables(W, p, d):
    n = p["pda_states"] * 256
    return (W["pda_next"][d["next"] // 2:][:n].reshape(-1, 256).tolist(), W["pda_act"][d["act"] // 2:][:n].reshape(-1, 256).tolist(),
            W["pda_flags"][d["flags"]:][:p["pda_states"]])


def ref_pda_mask(W, p, bug=None):
    V = p["V"]
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        d = W["pda"][slot]
        if W["slots"][slot]["finish"] or d["next"] == -1:
            continue
        nxt, act, _ = pda_tables(W, p, d)
        depth = min(max(int(d["depth"]), 0), MAX_DEPTH)
        base = [int(x) for x in d["stack"][:depth]]
        if bug == "stack_stage_64":
            base = [x if i < 32 else 0 for i, x in enumerate(base)]
        seen = {}
        x = W["logits"][row]
        for v in range(V):
            word = token_word(W, p, v) if v > 0 else None
            if not word:
                x[v] = -INF
                continue
            if word not in seen:
                seen[word] = pda_walk(nxt, act, int(d["max_depth"]), int(d["state"]), base, word, 9 if bug == "span_9" else SPAN)[0]
            if not seen[word]:
                x[v] = -INF


def dfa_update(W, p, row, slot, tok):
    if "dfa" not in W:
        return False
    d = W["dfa"][slot]
    if d["trans"] == -1:
        return False
    e = int(W["tok_end"].reshape(p["n_rows"], p["V"])[row, tok]) if 0 <= tok < p["V"] else 0
    if not e:
        return False
    d["state"] = e
    fl = int(W["dfa_flags"][d["flags"] + e])
    return bool(fl & 1) and (int(d["mode"]) == 1 or bool(fl & 2))


def pda_update(W, p, slot, tok):
    if "pda" not in W:
        return False
    d = W["pda"][slot]
    if d["next"] == -1:
        return False
    word = token_word(W, p, tok) if 0 < tok < p["V"] else None
    if not word:
        return False
    nxt, act, flags = pda_tables(W, p, d)
    q, st, low = pda_walk(nxt, act, int(d["max_depth"]), int(d["state"]), [int(x) for x in d["stack"][:int(d["depth"])]], word)
    if not q:
        return False
    d["stack"][low:len(st)] = st[low:]                             # the entries the token owns; what lies above the new depth keeps its bits
    d["state"], d["depth"] = q, len(st)
    fl = int(flags[q])
    return len(st) == 0 and bool(fl & 1) and (int(d["mode"]) == 1 or bool(fl & 2))


def ref_post(W, p, bug=None):
    V, B = p["V"], p["max_batch"]
    k = int(W["run_step"][0])
    exempt = []
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        g = W["slots"][slot]
        tok = int(W["samp_tok"][row])
        if g["kind"] != 2:
            W["penalty"][slot] = decay_row(W["penalty"][slot].view(U32), tok, g["decay"], g["frequency"], g["presence"], bug).view(F32)
        if g["finish"]:
            exempt.append(slot)
            continue
        halt = dfa_update(W, p, row, slot, tok) or pda_update(W, p, slot, tok)
        prob = W["samp_prob"][row]
        W["out_tok"][k * B + slot] = tok & 0xFFFFFFFF
        W["out_prob"][k * B + slot] = prob
        if p["mixed"]:
            W["held"][slot] = tok
        else:
            at = slot if bug == "feedback_slot" else row
            if at < W["feedback"].size:
                W["feedback"][at] = tok
            else:
                W["_guard"] = ("feedback", -1)                     # the mistake writes behind the buffer: shown as a changed guard element
        if "topn_n" in W and W["topn_n"][slot] > 0:
            m, lns = W["side_ms"][2 * row], W["side_ms"][2 * row + 1]
            xt = W["side_rows"][row * V + tok] if 0 <= tok < V else F32(-INF)
            with np.errstate(invalid="ignore"):
                W["tok_logp"][k * B + slot] = lns if np.isnan(lns) else F32(-INF) if xt == -INF else F32(F32(xt - m) - lns)
        g["draws"] += 1
        g["emitted"] += 1
        if g["kind"] == 2:
            g["tau"] = mirostat(g["tau"], prob, g["miro_target"], g["miro_rate"])
        stop = tok == 0 or any(int(g["stop"][j]) == (tok & 0xFFFFFFFF) for j in range(int(g["n_stop"])))
        at_max = g["emitted"] > g["max_tokens"] if bug == "max_lt" else g["emitted"] >= g["max_tokens"]
        st = W["stops"][slot] if "stops" in W else None
        if st is None or st["n_str"] <= 0:
            fin = 1 if halt or stop else 2 if at_max else 0
        else:                                                      # the reference's `process` for this one token, the bounded buffer put in
            strs = [bytes(st["str"][j][:min(int(st["len"][j]), 128)]) for j in range(min(int(st["n_str"]), 8))]
            tail = bytes(st["buf"][:int(st["buf_len"])])
            word = token_word(W, p, tok)
            fin, _, after = stop_expected(strs, [(0 if halt or stop else 1, word)], 1 if at_max else 2, tail, 0)[0]
            if fin == 0:
                st["buf"][:len(after)] = np.frombuffer(after, U8)
                st["buf_len"] = len(after)
        if fin:
            g["freeze_at"], g["finish"] = k, fin
    W["_exempt"] = exempt


def topn_write(W, row, x, n, ids_at, ids_role, logp_role, ms_role, rows_role, V):
    ids, lp = TN.topn_ref(x, n)
    m, lns = TN.lse64(x)
    if np.isnan(lp).all():
        lns = np.nan
    W[ids_role][ids_at:ids_at + n] = ids
    W[logp_role][ids_at:ids_at + n] = lp.astype(F32)
    W[ms_role][2 * row:2 * row + 2] = (F32(m), F32(lns))
    W[rows_role][row * V:(row + 1) * V] = x


def ref_topn(W, p, bug=None):
    V, B = p["V"], p["max_batch"]
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        n = int(W["topn_n"][slot])
        if n <= 0 or n > TOPN_MAX or W["slots"][slot]["finish"]:
            continue
        k = int(W["run_step"][0]) + (0 if p["mixed"] or bug == "topn_at_run_step" else 1)
        topn_write(W, row, W["logits"][row], n, (k * B + slot) * TOPN_MAX, "top_ids", "top_logp", "side_ms", "side_rows", V)


def ref_topn_pair(W, p, bug=None):
    ref_topn(W, p, bug)
    for row in range(p["n_rows"]):
        topn_write(W, row, W["logits"][row], p["n"], row * p["n"], "out_ids2", "out_logp2", "side_ms2", "side_rows2", p["V"])


def state_parts(W, p, slot):
    nsx, nw = p["nsx"], p["nw"]
    return np.concatenate([W["sxa"][slot * nsx:(slot + 1) * nsx], W["sxf"][slot * nsx:(slot + 1) * nsx], W["wkv"][slot * nw:(slot + 1) * nw]])


def ref_freeze(W, p, bug=None):
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        g = W["slots"][slot]
        if not g["finish"] or (g["freeze_at"] != W["run_step"][0] and bug != "freeze_always") or W["shadow"][slot] == -1:
            continue
        at = int(W["shadow"][slot])
        W["shadow_mem"][at:at + 2 * p["nsx"] + p["nw"]] = state_parts(W, p, slot)


def ref_capture(W, p, bug=None):
    V = p["V"]
    for row in range(p["n_rows"]):
        slot = slot_of(W, p, row, bug)
        c, g = W["cap"][slot], W["slots"][slot]
        p_row = int(c["p_row"]) if p["mixed"] else -1              # the decode-only instantiation does not look at p_row
        if (c["f_row"] == -1 and p_row == -1) or (g["finish"] and bug != "capture_rider"):
            continue
        prompt = p_row != -1 and g["draws"] == 0
        if c["f_row"] != -1:
            W["cap_mem"][int(c["f_row"]):][:V] = W["logits"][row]
        if prompt:
            W["cap_mem"][p_row:][:V] = W["logits"][row]
            W["cap_mem"][int(c["p_state"]):][:2 * p["nsx"] + p["nw"]] = state_parts(W, p, slot)


def ref_inject(W, p, bug=None):
    for row in range(p["first_row"], p["n_rows"]):
        src = int(W["cap"][slot_of(W, p, row, bug)]["inj_row"])
        if src != -1:
            W["logits"][row] = W["cap_mem"][src:src + p["V"]]


def rec_bytes(B):
    return (8 + 12 * B + 15) & ~15                                 # gen_watch.h: u64 stamp | u32 tok[B] | f32 prob[B] | i32 finish[B], padded to 16 bytes


def ring_bytes(steps, B):
    return steps * rec_bytes(B) + 16 + 4 * B                       # records | u64 head (padded to 16 bytes) | u32 cancel[B]


def ref_publish(W, p, bug=None):
    w = W["watch"][0]
    if w["ring"] == -1:
        return
    B, steps, k = p["max_batch"], p["ring_steps"], int(W["run_step"][0])
    seq = int(w["seq"])
    ring = W["ring"]
    cancel = ring[steps * rec_bytes(B) + 16:][:4 * B].view(U32)
    rec = ring[(seq % steps) * rec_bytes(B):][:rec_bytes(B)]
    payload = rec[8:8 + 12 * B].view(U32)
    for b in range(B):
        tok, prob = (int(W["out_tok"][k * B + b]), int(W["out_prob"].view(U32)[k * B + b])) if k >= 0 else (NO_TOKEN, 0xFFFFFFFF)
        g = W["slots"][b]
        fin = int(g["finish"])
        if fin == 0 and (tok != NO_TOKEN or bug == "cancel_no_draw") and cancel[b] != 0:
            fin = 4
            g["freeze_at"], g["finish"] = k, fin
        payload[b], payload[B + b], payload[2 * B + b] = tok, prob, fin
    rec[:8].view(np.uint64)[0] = seq if bug == "stamp_seq" else seq + 1
    ring[steps * rec_bytes(B):][:8].view(np.uint64)[0] = seq + 1
    w["seq"] = seq + 1


def ref_tokens(W, p, bug=None):
    W["run_step"][0] += 1
    for r in range(p["T"]):
        if W["token"][r] < 0:
            W["token"][r] = W["held"][W["row_slot"][r]]


def ref_handover(W, p, bug=None):
    for r in range(p["T"]):
        if p["to_held"]:
            W["held"][W["row_slot"][r]] = W["feedback"][r]
        else:
            W["feedback"][r] = W["held"][W["row_slot"][r]]


def sample(x, sp):
    """launch_nucleus on one row: tests/sample_cases.py's emulate / draw on a family A row (one value on 2^e ids), where token and out_prob are exact.
    Src asserts the family: the table's images are made so that the EDITED row is such a row."""
    from tests import sample_cases as SC
    r = SC.row(None, int(sp["kind"]) & 3, float(sp["uniform"]), top_k=int(sp["top_k"]), top_p=float(sp["top_p"]), T=float(sp["temperature"]), tau=float(sp["tau"]),
               wide=bool(int(sp["kind"]) & 4))
    tok, prob = SC.expect(SC.Src(x, "A"), r)
    return int(tok), F32(prob)


def ref_step(W, p, bug=None, image=None):
    """N whole steps in the engine's order (rwkv_engine.cpp gen_sample and the mixed step around it); the logits block is this step's image
    in front of each.  `image(i, W)` makes the image from the state in front of step i (how the table's images come to be)."""
    N, V, n = p["n_steps"], p["V"], p["n_rows"]
    imgs = W["logits_steps"].reshape(N, n, V)
    token0 = W["token"].copy() if "token" in W else None
    exempt = set()
    for i in range(N):
        if "watch" in W and i == p["cancel_step"]:                 # the host side of the watch: the slot's request goes away between two steps
            W["ring"][p["ring_steps"] * rec_bytes(p["max_batch"]) + 16:].view(U32)[p["cancel_slot"]] = 1
        if image is not None:
            imgs[i] = image(i, W)
        W["logits"][:] = imgs[i]
        if p["mixed"]:
            W["token"][:] = token0
            ref_tokens(W, p)
        if "cap" in W and p["mixed"] and p["first_row"] < n:
            ref_inject(W, p)
        if "cap" in W:
            ref_capture(W, p)
        if "topn_n" in W:
            ref_topn(W, p)
        ref_pre(W, p)
        if "dfa" in W:
            ref_mask(W, p)
        if "pda" in W:
            ref_pda_mask(W, p)
        rows = W["rows"].view(SP_DT)
        for r in range(n):
            W["samp_tok"][r], W["samp_prob"][r] = sample(W["logits"][r], rows[r])
        ref_post(W, p)
        exempt |= set(W["_exempt"])
        if "watch" in W:
            ref_publish(W, p)
        ref_freeze(W, p)
    W["_exempt"] = sorted(exempt)


REF = {"step": ref_step, "gen_pre": ref_pre, "gen_topn": ref_topn, "gen_mask": ref_mask, "gen_post": ref_post, "gen_publish": ref_publish, "gen_freeze": ref_freeze,
       "gen_capture": ref_capture, "gen_inject": ref_inject, "gen_tokens": ref_tokens, "gen_handover": ref_handover, "topn_pair": ref_topn_pair,
       "gen_pda_mask": ref_pda_mask}


def expected_world(c, d, bug=None):
    W = copy.deepcopy(d["W"])
    REF[KIND_NAME[c.kind]](W, c.p, bug)
    for role, names in POINTERS.items():
        if role in W:
            for nm in names:
                W[role][nm] = 0
    if "shadow" in W:
        W["shadow"][:] = 0
    return W


def reference_results(c, d, bug=None):
    """What a correct launch returns (with `bug`: what a kernel with that one-line mistake returns): every buffer whole."""
    W = expected_world(c, d, bug)
    res = {}
    for b in d["bufs"]:
        img = image_of(b).copy()
        own(dict(x=img), Buf("x", b.esize, 1, b.n, b.off))[:] = words(W[b.role])
        res[b.role] = img
    if "_guard" in W:
        role, _ = W["_guard"]
        res[role][GUARD - 1] ^= 1                                  # the last element of the front guard band
    return res, W


def check_case(c, d, res, line, ratios=None):
    """Findings as strings; `ratios` collects (case, what, worst top-n error / bound)."""
    msgs, worst = [], 0.0
    if line != plan_line(c):
        msgs.append(f"{c.name}: the probe ran {line}, the table says {plan_line(c)}")
    want, W = reference_results(c, d)
    V = c.p["V"]
    for b in d["bufs"]:
        got, exp = res[b.role], want[b.role]
        differ = got != exp
        # the places the reference writes with logf / expf behind them: numeric, at topn_cases' bound (m of side_ms: exact).  In kind
        # step tok_logp is one of them: gen_post forms it from the ln S the device's own gen_topn left.
        tolerant = b.role in TOLERANT or (b.role == "tok_logp" and KIND_NAME[c.kind] == "step")
        if b.role in ("logits", "penalty") and differ.any():
            # a NaN the launch COMPUTES (a penalty entry that is a NaN other than GEN_ABSENT is an entry like any other): the payload a NaN
            # operand leaves in a sum or product is the hardware's, so such a cell must hold a NaN — in a penalty row one that is still an entry
            made = (exp != image_of(b)) & np.isnan(exp.view(F32))
            differ &= ~(made & np.isnan(got.view(F32)) & ((got != ABSENT) | (b.role != "penalty")))
        if tolerant and differ.any():
            wrote = exp != image_of(b)
            g, e = got.view(F32).astype(F64), exp.view(F32).astype(F64)
            with np.errstate(invalid="ignore"):
                bound = TN.FP32_TOL * np.maximum(1.0, np.abs(e))
                err = np.where(np.isnan(e), np.where(np.isnan(g), 0.0, INF), np.where(np.isinf(e), np.where(g == e, 0.0, INF), np.abs(g - e)))
                err = np.where(np.isnan(err), INF, err)
            if b.role.startswith("side_ms"):
                at = np.arange(got.size) - GUARD - b.off
                bound = np.where(at % 2 == 0, 0.0, bound)          # (m, ln S): m is the row's maximum, exactly
            ok = wrote & (err <= bound)
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(wrote & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
            worst = max(worst, float(q.max()))
            differ &= ~ok
        if b.role == "penalty" and W.get("_exempt"):               # the one exemption: the row of a slot that had finished before this gen_post
            keep = np.ones(got.size, bool)
            for s in W["_exempt"]:
                keep[GUARD + s * V:GUARD + (s + 1) * V] = False
            differ &= keep
        if differ.any():
            i = int(np.nonzero(differ)[0][0])
            at = i - GUARD - b.off
            where = "a guard band or spare row" if at < 0 or at >= b.n - 2 * b.off else f"element {at}"
            msgs.append(f"{c.name}: {b.role}: {int(differ.sum())} elements differ, first at {where}: got {int(got[i]):#x}, want {int(exp[i]):#x}")
    if KIND_NAME[c.kind] == "topn_pair":                            # gen_topn and launch_topn_rows on the same rows: the same bits
        bo = {b.role: b for b in d["bufs"]}
        n, B = c.p["n"], c.p["max_batch"]
        k = int(d["W"]["run_step"][0]) + (0 if c.p["mixed"] else 1)
        for row in range(c.p["n_rows"]):
            slot = slot_of(d["W"], c.p, row)
            if d["W"]["topn_n"][slot] != n or d["W"]["slots"][slot]["finish"]:
                continue
            at = (k * B + slot) * TOPN_MAX
            for a, b2, lo, ln in (("top_ids", "out_ids2", at, n), ("top_logp", "out_logp2", at, n), ("side_ms", "side_ms2", 2 * row, 2), ("side_rows", "side_rows2", row * V, V)):
                x, y = own(res, bo[a])[lo:lo + ln], own(res, bo[b2])[(row * n if a.startswith("top") else lo):][:ln]
                if (x != y).any():
                    msgs.append(f"{c.name}: row {row}: {a} of gen_topn and {b2} of launch_topn_rows differ in bits")
    if ratios is not None:
        ratios.append((c.name, c.name, worst))
    return msgs


# ------------------------------------------------------------------------------------------------
# worlds
# ------------------------------------------------------------------------------------------------
def geom(B, mixed):
    """(row_slot, out_rows, riders): a non-identity arrangement with gaps, n_rows < max_batch where max_batch > 1; with five slots a finished
    rider (slot 1) between two live rows; mixed: non-adjacent step rows out of a longer step, one slot in mid-prefill without a logits row.
    72 slots, the width of a server's engine: 33 logits rows (past a wavefront's 32) over a scattered slot list that reaches into the second word
    of a slot mask (63, 64, 71), two finished riders; mixed: 70 step rows — 33 decode rows around a 20-token prompt that ends and 17 rows of a
    slot in mid-prefill — and 34 output rows."""
    if B == WIDE_B:
        wide = [71, 63, 64] + [s for s in ((5 * i + 2) % WIDE_B for i in range(WIDE_B)) if s not in (71, 63, 64, 10, 40)][:30]
        riders = [wide[1], wide[17]]
        if not mixed:
            return wide, None, riders
        rs, orows = [], []
        for i, s in enumerate(wide):
            if i in (10, 22):                                      # slot 10: a prompt that ends here (its last row is sampled); slot 40: in mid-prefill, no logits row
                n, slot = ((20, 10), (17, 40))[i == 22]
                rs += [slot] * n
                orows += [len(rs) - 1] if i == 10 else []
            orows.append(len(rs))
            rs.append(s)
        return rs, orows, riders
    if not mixed:
        return {1: ([0], None, []), 3: ([2, 0], None, []), 5: ([4, 1, 3], None, [1])}[B]
    return {1: ([0, 0, 0], [2], []), 3: ([2, 2, 1, 0, 0], [1, 4], []), 5: ([4, 4, 1, 0, 3, 3, 0], [1, 2, 5], [1])}[B]


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def params(**kw):
    p = {k: 0 for k in PARAMS}
    p["cancel_step"] = -1
    p.update(kw)
    return p


def base_world(name, V, B, mixed, run_step=0):
    rng = rng_of(name)
    rs, orows, riders = geom(B, mixed)
    s = np.zeros(B, SLOT_DT)
    s["top_p"], s["top_k"], s["temperature"], s["tau"] = 0.5, 128, 1.0, 0.5
    s["presence"], s["frequency"], s["decay"] = 0.3, 0.3, 0.99654026
    s["miro_target"], s["miro_rate"] = 3.0, 0.1
    s["seed"] = rng.integers(0, 1 << 63, B, dtype=np.uint64) * 2 + 1
    s["stream"], s["draws"] = rng.integers(0, 1 << 32, B, dtype=np.uint64), rng.integers(0, 1000, B)
    s["max_tokens"], s["emitted"], s["freeze_at"] = 100, 5, -1
    s["kind"] = np.arange(B) % 3
    for r in riders:
        s["finish"][r], s["freeze_at"][r] = 1, run_step - 1
    W = {"slots": s, "row_slot": np.array(rs, I32), "run_step": np.array([run_step], I32)}
    if mixed:
        W["out_rows"] = np.array(orows, I32)
    n_rows = len(orows) if mixed else len(rs)
    return W, rng, params(V=V, max_batch=B, n_rows=n_rows, T=len(rs), mixed=int(mixed)), riders


def row_slots(W, p):
    return [slot_of(W, p, r) for r in range(p["n_rows"])]


def penalty_rows(rng, B, V):
    pen = rng.uniform(0.1, 2.0, (B, V)).astype(F32)
    pen.view(U32)[rng.random((B, V)) < 0.3] = ABSENT
    pen.view(U32)[:, 9] = 0x7FC00000                               # a NaN that is not GEN_ABSENT: an entry (membership is by the bit pattern)
    return pen


def logits_rows(rng, n, V):
    x = (rng.standard_normal((n, V)) * 3).astype(F32)
    x[:, V // 3] = -INF
    x[:, 5] = -0.0                                                 # with no entry and a zero bias it stays -0.0
    return x


def pre_world(name, V, B, mixed, var):
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=(-1, 6)[var % 2])
    s = W["slots"]
    s["kind"] = (np.arange(B) + var) % 3
    s["has_bias"] = [(b + var) % 2 for b in range(B)] if var != 1 else 0
    s["wide"] = [4 if b % 2 == 0 else 0 for b in range(B)]
    first = row_slots(W, p)[0]                                     # the first row: penalties and (but for var 1) a bias, so both associations matter
    s["kind"][first], s["has_bias"][first] = var % 2, int(var != 1)
    if V == 1024 and var != 1:                                     # a short row: every live row is needed for a hundred entries that tell
        for slot in row_slots(W, p):
            s["kind"][slot], s["has_bias"][slot] = slot % 2, 1
    W["logits"] = logits_rows(rng, p["n_rows"], V)
    W["penalty"] = penalty_rows(rng, B, V)
    W["penalty"].view(U32)[:, 5] = ABSENT
    if var != 1:                                                   # var 1: no slot has a bias and the bias pointer is null
        bias = rng.standard_normal((B, V)).astype(F32)
        bias[rng.random((B, V)) < 0.3] = 0.0
        bias[:, 5] = 0.0
        W["bias"] = bias
    W["rows"] = sent(p["n_rows"] * 6)
    return W, p


def token_table(words_of, n_tok):
    """tok_off [n_tok + 1], tok_bytes: words_of(i) -> bytes, or None for an id marked unknown."""
    off, data = np.zeros(n_tok + 1, U32), bytearray()
    for i in range(n_tok):
        w = words_of(i)
        off[i] = len(data) | (TOK_UNKNOWN if w is None else 0)
        data += w or b""
    off[n_tok] = len(data)
    return off, np.frombuffer(bytes(data) + b"\0" * 16, U8).copy()


ALPHA = b"ab[](){}\",:1 "


def random_words(rng, n_tok, alphabet=ALPHA, special=None):
    """lengths 0, 1 and 128 among short random words; id 7 (where there is one) is marked unknown."""
    special = dict(special or {})
    lens = rng.integers(1, 6, n_tok)
    pick = rng.integers(0, len(alphabet), (n_tok, 5))

    def w(i):
        if i in special:
            return special[i]
        if i == 7:
            return None
        if i % 97 == 3:
            return b""
        if i % 97 == 4:
            return bytes(alphabet[j % len(alphabet)] for j in range(i, i + 128))
        return bytes(alphabet[j] for j in pick[i][:lens[i]])
    return w


def random_dfa(rng, nq=6):
    trans = np.zeros((nq, 256), U16)
    for q in range(1, nq):
        for ch in ALPHA:
            trans[q, ch] = rng.integers(0, nq) if rng.random() < 0.8 else 0
    accepting = rng.integers(0, 2, nq).astype(U8)
    flags = np.array([(1 if q and accepting[q] else 0) | (0 if (trans[q] != 0).any() else 2) for q in range(nq)], U8)
    flags[nq - 1] |= 1
    return trans, flags


def mask_world(name, V, B, mixed, n_tok):
    W, rng, p, riders = base_world(name, V, B, mixed)
    trans, flags = random_dfa(rng)
    p.update(n_tok=n_tok, dfa_states=trans.shape[0])
    W["tok_off"], W["tok_bytes"] = token_table(random_words(rng, n_tok), n_tok)
    W["dfa_trans"], W["dfa_flags"] = trans.reshape(-1), flags
    d = np.zeros(B, DFA_DT)
    d["trans"], d["flags"] = -1, -1
    slots = row_slots(W, p)
    for i, s in enumerate(slots):
        if i != 1 or s in riders:                                  # the second row's slot is unconstrained (or a rider that is constrained)
            d[s] = (0, 0, 2 + i % 3, i % 2)                        # a start state other than the table's first
    W["dfa"] = d
    W["logits"] = logits_rows(rng, p["n_rows"], V)
    W["tok_end"] = np.full(p["n_rows"] * V, 0x7EAD, U16)
    return W, p


def bracket_pda():
    """Hand-made: '[' pushes return state 1, '(' pushes return state 2, ']' and ')' pop, 'a' is plain; states 1 and 2 behave alike and accept."""
    nxt, act = np.zeros((3, 256), U16), np.zeros((3, 256), U16)
    for q in (1, 2):
        nxt[q, ord("a")] = q
        nxt[q, ord("[")], act[q, ord("[")] = 1, 1
        nxt[q, ord("(")], act[q, ord("(")] = 2, 2
        act[q, ord("]")] = act[q, ord(")")] = POP
    accepting = np.array([0, 1, 1], U8)
    return nxt, act, accepting


def pda_flags(nxt, act, accepting):
    return np.array([(1 if q and accepting[q] else 0) | (0 if ((act[q] != POP) & (nxt[q] != 0)).any() else 2) for q in range(nxt.shape[0])], U8)


def json_pda():
    """The project's own RFC 8259 automaton (rwkv_pda_json through runtime.py; host only)."""
    from ai00_server_amd import build, runtime as rt
    build.build(verbose=False)
    return rt.Pda.json().table()


PDA_SPECIAL = {1: b"[" * 8, 2: b"[" * 9, 3: b"][", 4: b"]", 5: b"[[", 6: b"]]]" + b"(" * 8, 8: b"a", 9: b"]]" + b"[(" * 4 + b"(", 10: b")", 11: b"(" * 7 + b"]" * 7 + b"[" * 8}


def pda_world(name, V, B, mixed, n_tok, table, configs):
    """configs: per logits row (state, stack, max_depth, mode) or None for an unconstrained slot."""
    W, rng, p, riders = base_world(name, V, B, mixed)
    nxt, act, accepting = bracket_pda() if table == "bracket" else json_pda()
    p.update(n_tok=n_tok, pda_states=nxt.shape[0])
    alphabet = b"a[]()" if table == "bracket" else b"{}[]\",:0 tre"
    W["tok_off"], W["tok_bytes"] = token_table(random_words(rng, n_tok, alphabet, PDA_SPECIAL if table == "bracket" else None), n_tok)
    W["pda_next"], W["pda_act"], W["pda_flags"] = nxt.reshape(-1).copy(), act.reshape(-1).copy(), pda_flags(nxt, act, accepting)
    d = np.zeros(B, PDA_DT)
    d["next"], d["act"], d["flags"] = -1, -1, -1
    d["stack"] = 0x7EAD
    for i, s in enumerate(row_slots(W, p)):
        cfg = configs[i % len(configs)]
        if cfg is None and s not in riders:
            continue
        state, stack, max_depth, mode = cfg or configs[0]
        d[s]["next"], d[s]["act"], d[s]["flags"] = 0, 0, 0
        d[s]["stack"][:len(stack)] = stack
        d[s]["state"], d[s]["depth"], d[s]["mode"], d[s]["max_depth"] = state, len(stack), mode, max_depth
    W["pda"] = d
    W["logits"] = logits_rows(rng, p["n_rows"], V)
    return W, p


def json_config(text, max_depth=64):
    from ai00_server_amd import runtime as rt
    q, st = rt.Pda.json(max_depth=max_depth).walk(text)
    assert q
    return (q, st, max_depth, 0)


POST_TOKS = (0, 1, 2, 3, 1023, 1024, 16383, 16384)                 # each lane of a float4, both sides of a block and of a pass; V - 1 is added per V


def fused_differs(pv, decay, freq):
    return F32(F64(pv) * F64(decay) + F64(freq)) != F32(F32(pv * decay) + freq)


def post_world(name, V, B, mixed, var, with_dfa=False, with_topn=False, with_pda=False, at=None):
    run_step = (0, 7)[var % 2]
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=run_step)
    steps = 9
    p.update(steps=steps)
    s = W["slots"]
    n_rows = p["n_rows"]
    toks = [t for t in POST_TOKS + (V - 1,) if t < V]
    tok = np.array([toks[(var * 3 + r) % len(toks)] for r in range(n_rows)] if at is None else at, I32)   # at: the drawn token of every row, given
    W["penalty"] = penalty_rows(rng, B, V)
    W["samp_tok"], W["samp_prob"] = tok, rng.uniform(0.5, 9.0, n_rows).astype(F32)
    for r, slot in enumerate(row_slots(W, p)):
        sc = (var + r) % 7                                         # the bookkeeping scenario of the row
        if sc == 1 and at is not None:
            sc = 6
        g = s[slot]
        g["kind"] = 2 if sc in (4, 5) else r % 2
        g["n_stop"] = 8 if sc in (0, 3, 6) else 0
        g["stop"] = [70000 + j for j in range(8)]
        if sc in (0, 3):
            g["stop"][7] = tok[r]                                  # the hit is the last entry
        if sc == 1:
            tok[r] = 0                                             # token 0 stops
        if sc in (2, 3):
            g["max_tokens"] = g["emitted"] + 1                     # 2: LENGTH; 3: stop and max together: STOP
        if sc == 4:
            g["tau"], W["samp_prob"][r] = 6.0, 2.0                 # max_surprise - rate * (2 - 3) = 6.1 < 12
        if sc == 5:
            g["tau"], g["miro_rate"], W["samp_prob"][r] = 11.5, 1.0, 0.25   # 11.5 + 2.75 > 12: the clamp
        if g["kind"] != 2 and 0 <= tok[r] < V and (r + var) % 3 != 2:   # the drawn token has an entry on which fusing changes the bits
            pv = F32(rng.uniform(0.1, 2.0))
            while not fused_differs(pv, g["decay"], g["frequency"]):
                pv = F32(rng.uniform(0.1, 2.0))
            W["penalty"][slot, tok[r]] = pv
        elif g["kind"] != 2 and 0 <= tok[r] < V:
            W["penalty"].view(U32)[slot, tok[r]] = ABSENT          # no entry: it becomes `presence`
    W["out_tok"], W["out_prob"] = sent(steps * B), sent(steps * B).view(F32)
    W["held" if mixed else "feedback"] = sent(B if mixed else n_rows).view(I32)
    if with_topn:
        W["topn_n"] = np.array([(3, 0, 32, 1, 5)[b % 5] for b in range(B)], I32)
        W["tok_logp"] = sent(steps * B).view(F32)
        W["side_rows"] = logits_rows(rng, n_rows, V).reshape(-1)
        ms = np.stack([rng.uniform(1.0, 9.0, n_rows), rng.uniform(0.5, 3.0, n_rows)], 1).astype(F32)
        if var % 2:
            ms[0, 1] = np.nan                                      # a poisoned row: NaN passes through
        else:
            W["side_rows"][tok[0]] = -INF                          # the drawn token's raw logit is -inf
        W["side_ms"] = ms.reshape(-1)
    if with_dfa:
        trans, flags = random_dfa(rng)
        p.update(dfa_states=trans.shape[0])
        W["dfa_trans"], W["dfa_flags"] = trans.reshape(-1), flags
        d = np.zeros(B, DFA_DT)
        d["trans"], d["flags"] = -1, -1
        ends = rng.integers(1, trans.shape[0], (n_rows, V)).astype(U16)
        for r, slot in enumerate(row_slots(W, p)):
            if r != 1:
                d[slot] = (0, 0, 2, (var + r) % 2)
                ends[r, tok[r]] = (trans.shape[0] - 1) if (var + r) % 3 else 0   # the accepting state, or: the token was not allowed
        W["dfa"], W["tok_end"] = d, ends.reshape(-1)
    if with_pda:
        nxt, act, accepting = bracket_pda()
        n_tok = min(V, 1024)
        p.update(n_tok=n_tok, pda_states=3)
        sp = dict(PDA_SPECIAL)
        cfgs = [(b"[(", [1, 2, 1]), (b"]", [2, 1]), (b"]", [2]), (b"[" * 9, [1]), (b"][", [2, 1, 2])]   # push, pop, pop to depth 0 (halts), not allowed, pop below then push
        for r in range(n_rows):
            if 0 < tok[r] < n_tok:
                sp[int(tok[r])] = cfgs[(var + r) % len(cfgs)][0]
        W["tok_off"], W["tok_bytes"] = token_table(random_words(rng, n_tok, b"a[]()", sp), n_tok)
        W["pda_next"], W["pda_act"], W["pda_flags"] = nxt.reshape(-1).copy(), act.reshape(-1).copy(), pda_flags(nxt, act, accepting)
        d = np.zeros(B, PDA_DT)
        d["next"], d["act"], d["flags"], d["stack"] = -1, -1, -1, 0x7EAD
        for r, slot in enumerate(row_slots(W, p)):
            if r != 1:
                st = cfgs[(var + r) % len(cfgs)][1]
                d[slot]["next"], d[slot]["act"], d[slot]["flags"] = 0, 0, 0
                d[slot]["stack"][:len(st)] = st
                d[slot]["state"], d[slot]["depth"], d[slot]["mode"], d[slot]["max_depth"] = 1, len(st), (var + r) % 2, 64
        W["pda"] = d
    return W, p


def stop_slot(strs, tail, n_str=None):
    st = np.zeros(1, STOP_DT)[0]
    st["str"][:], st["buf"][:] = 0xAD, 0xAD
    for j, x in enumerate(strs):
        st["str"][j][:len(x)] = np.frombuffer(x, U8)
        st["len"][j] = len(x)
    st["buf"][:len(tail)] = np.frombuffer(tail, U8)
    st["n_str"], st["buf_len"] = len(strs) if n_str is None else n_str, len(tail)
    return st


FILL = [bytes([0x80 + j]) * 3 for j in range(8)]                   # eight strings that match nothing of the ASCII traffic below
LONG = bytes(range(33, 33 + 94)) + bytes(range(33, 33 + 34))       # 128 bytes
# name -> (strings, tail, the drawn token's bytes or None = an unknown id, extra).  What each is for stands beside it.
STOP_SCENES = {
    "began_three_tokens_ago": ([b"<END>"], b"xy<EN", b"D>"),        # a match that ends in this token and began in the buffer
    "string7_alone": (FILL[:7] + [b"stop"], b"..st", b"op"),        # the hit in lane 7 alone: all three DPP stages carry it down
    "equal_1_and_5": ([FILL[0], b"halt", FILL[2], FILL[3], FILL[4], b"halt", FILL[6], FILL[7]], b"ha", b"lt!"),   # equal results across the two quads
    "equal_3_and_4": (FILL[:3] + [b"halt", b"halt"] + FILL[5:], b"ha", b"lt"),                                  # equal results, lanes 3 and 4: the last stage
    "matched_beats_unmatched_same_place": ([b"abcd", b"ab"], b"zz", b"ab"),   # both candidates at index 2; the matched one wins although it stands later
    "earlier_unmatched_loses": ([b"bcq", b"cd"], b"a", b"bcd"),
    "len128": ([LONG], LONG[:100], LONG[100:]),                    # a 128-byte string
    "fits_512": ([b"never"], b"x" * 500, b"y" * 12),               # buf_len + wlen == 512: fits
    "hands_back_513": ([b"never"], b"x" * 500, b"y" * 13),         # 513: RWKV_GEN_HANDBACK, the buffer unchanged
    "unknown_id": ([b"never"], b"abc", None),                      # `tokenizer.decode` failed: empty word, STOP
    "empty_token": ([b"never"], b"abc", b""),
    "utf8_split_held": ([b"never"], b"", b"a\xe4\xbd"),            # the head is not valid UTF-8: held back, the buffer kept whole
    "utf8_split_released": ([b"never"], b"a\xe4\xbd", b"\xa0b"),   # the second case: the character completes and the head leaves
    "no_strings": ([], b"", b"hello"),                             # a slot without strings inside a `stops` launch: the token-stop path
    "finishes_at_max": ([b"never"], b"keep", b"me"),               # a slot that finishes leaves buf / buf_len as they were
    "partial_kept": ([b"<END>"], b"", b"ab<E"),                    # the tail that may still become a match stays
}


def stops_world(name, V, B, mixed, scenes):
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=2)
    p.update(steps=4, n_tok=V)
    s = W["slots"]
    n_rows = p["n_rows"]
    slots = row_slots(W, p)
    special, tok = {}, np.zeros(n_rows, I32)
    for r in range(n_rows):
        tok[r] = 20 + 16 * r + r                                   # distinct ids, different float4 lanes
        special[int(tok[r])] = STOP_SCENES[scenes[r % len(scenes)]][2]
    W["tok_off"], W["tok_bytes"] = token_table(random_words(rng, V, ALPHA, special), V)
    st = np.zeros(B, STOP_DT)
    st["str"], st["buf"] = 0xAD, 0xAD
    for r, slot in enumerate(slots):
        sc = scenes[r % len(scenes)]
        st[slot] = stop_slot(STOP_SCENES[sc][0], STOP_SCENES[sc][1])
        s[slot]["kind"] = r % 2
        if sc == "finishes_at_max":
            s[slot]["max_tokens"] = s[slot]["emitted"] + 1
    W["stops"] = st
    W["penalty"] = penalty_rows(rng, B, V)
    W["samp_tok"], W["samp_prob"] = tok, rng.uniform(0.5, 9.0, n_rows).astype(F32)
    W["out_tok"], W["out_prob"] = sent(4 * B), sent(4 * B).view(F32)
    W["held" if mixed else "feedback"] = sent(B if mixed else n_rows).view(I32)
    return W, p


STEP_SCENES = ("penalties_bias_stop", "topn_capture_rider", "mixed_prompt_item_prefill", "dfa_beside_pda", "watch_cancel", "wide_72")


def step_world(name, scene):
    """Three whole steps.  The images are made step by step from the state the reference has reached (ref_step's `image`): raw rows such that
    the row gen_pre and the masks leave is 1.5 on 2^e ids and -inf elsewhere.  Penalties and biases are small dyadic numbers, so every
    compensation x = 1.5 - ((-p) + b) is exact."""
    V, N = 1024, 3
    mixed = scene == "mixed_prompt_item_prefill"
    B = WIDE_B if scene == "wide_72" else 5 if scene in ("penalties_bias_stop", "mixed_prompt_item_prefill") else 3
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=-1)
    steps = N + 1
    p.update(steps=steps, n_steps=N, nsx=64, nw=64, first_row=p["n_rows"])
    s = W["slots"]
    s["presence"], s["frequency"], s["decay"] = 0.5, 0.25, 0.5
    s["miro_target"], s["miro_rate"], s["tau"] = 3.0, 0.5, 6.0
    s["top_k"], s["top_p"], s["emitted"], s["max_tokens"] = 64, 0.75, 0, 100
    s["kind"] = 0
    if mixed:
        W["out_rows"] = np.array([1, 5, 2], I32)                   # slots 4, 3, 1; slot 0 is in mid-prefill and has no logits row
        s["finish"], s["freeze_at"] = 0, -1
        W["token"], W["held"] = np.array([11, 12, -1, 13, 14, -1, 15], I32), np.array([21, 22, 23, 24, 25], I32)
    slots = row_slots(W, p)
    n = p["n_rows"]
    W["penalty"] = np.full((B, V), ABSENT, U32).view(F32)
    pen = rng.choice([0.25, 0.5, 0.75, 1.0], (B, V)).astype(F32)
    keep = rng.random((B, V)) < 0.5
    W["penalty"][keep] = pen[keep]
    W["rows"] = np.zeros(n, SP_DT)
    W["rows"]["temperature"] = 1.0                                 # the inert row: what a rider of a decode-only step keeps
    W["rows"] = W["rows"].view(U32).reshape(-1)
    W["samp_tok"], W["samp_prob"] = sent(n).view(I32), sent(n).view(F32)
    W["out_tok"], W["out_prob"] = sent(steps * B), sent(steps * B).view(F32)
    W["held" if mixed else "feedback"] = W.get("held", sent(n).view(I32))
    W["logits"] = np.zeros((n, V), F32)
    W["logits_steps"] = np.zeros(N * n * V, F32)
    W["sxa"], W["sxf"], W["wkv"] = (rng.standard_normal(B * 64).astype(F32) for _ in range(3))
    W["shadow"], W["shadow_mem"] = np.arange(B, dtype=np.int64) * 192 + 64, sent(B * 192 + 64).view(F32)
    if scene == "penalties_bias_stop":
        s["kind"][slots[0]], s["kind"][slots[2]] = 0, 2
        s["has_bias"][slots[0]] = 1
        bias = rng.choice([0.0, 0.25, -0.5, 0.125], (B, V)).astype(F32)
        W["bias"] = bias
    if scene == "wide_72":                                         # 33 rows of 72 slots: every sampler kind, a bias on every second slot, the two riders from the start
        s["kind"], s["has_bias"] = np.arange(B) % 3, np.arange(B) % 2
        W["bias"] = rng.choice([0.0, 0.25, -0.5, 0.125], (B, V)).astype(F32)
        s["max_tokens"][slots[2]] = 2                              # finishes in step 1 (LENGTH), is frozen there and rides in step 2
    if scene == "topn_capture_rider":
        s["kind"][slots[0]], s["kind"][slots[1]] = 1, 0
        s["max_tokens"][slots[1]] = 2                              # finishes in step 1 (LENGTH) and rides in step 2
        W["topn_n"] = np.array([0, 0, 5], I32)
        W["top_ids"], W["top_logp"], W["tok_logp"] = sent(steps * B * TOPN_MAX), sent(steps * B * TOPN_MAX).view(F32), sent(steps * B).view(F32)
        W["side_ms"], W["side_rows"] = sent(n * 2).view(F32), sent(n * V).view(F32)
        cap = np.full(B * 4, -1, np.int64).view(CAP_DT)
        for b in slots:
            cap[b]["f_row"] = b * V                                # FINISH: the raw row of the step the slot finishes in stays
        W["cap"], W["cap_mem"] = cap, sent(B * V).view(F32)
    if mixed:
        p.update(first_row=2)
        s["kind"][1] = 2                                           # the item-armed slot: Mirostat leaves the injected row as it is
        s["draws"][4] = 0                                          # its prompt ends in step 0: draw 0, PROMPT capture
        cap = np.full(B * 4, -1, np.int64).view(CAP_DT)
        cap[4]["p_state"], cap[4]["p_row"], cap[1]["inj_row"] = 0, 192, 192 + V
        inj = np.full(V, -INF, F32)
        inj[rng.choice(np.arange(1, V), 8, replace=False)] = 1.5
        W["cap"], W["cap_mem"] = cap, np.concatenate([sent(192 + V).view(F32), inj])
    if scene == "dfa_beside_pda":
        trans, flags = random_dfa(rng)
        trans[1:, list(b"ab")] = np.maximum(trans[1:, list(b"ab")], 1)   # 'a' and 'b' lead on from every live state: no row is masked whole
        nxt, act, accepting = bracket_pda()
        p.update(n_tok=V, dfa_states=trans.shape[0], pda_states=3)
        W["tok_off"], W["tok_bytes"] = token_table(random_words(rng, V, b"ab[]()", PDA_SPECIAL), V)
        W["dfa_trans"], W["dfa_flags"] = trans.reshape(-1), flags & 1        # never END: the slot goes on for three steps unless it accepts with mode 1
        d = np.zeros(B, DFA_DT)
        d["trans"], d["flags"] = -1, -1
        d[slots[0]] = (0, 0, 2, 0)
        W["dfa"], W["tok_end"] = d, np.full(n * V, 0x7EAD, U16)
        W["pda_next"], W["pda_act"], W["pda_flags"] = nxt.reshape(-1).copy(), act.reshape(-1).copy(), pda_flags(nxt, act, accepting)
        q = np.zeros(B, PDA_DT)
        q["next"], q["act"], q["flags"], q["stack"] = -1, -1, -1, 0x7EAD
        q[slots[1]]["next"], q[slots[1]]["act"], q[slots[1]]["flags"] = 0, 0, 0
        q[slots[1]]["stack"][:2] = [1, 2]
        q[slots[1]]["state"], q[slots[1]]["depth"], q[slots[1]]["mode"], q[slots[1]]["max_depth"] = 1, 2, 0, 64
        W["pda"] = q
    if scene == "watch_cancel":
        ring_steps = 2
        p.update(ring_steps=ring_steps)
        ring = np.full(ring_bytes(ring_steps, B), 0xAD, U8)
        ring[ring_steps * rec_bytes(B):] = 0
        ring[ring_steps * rec_bytes(B) + 16:].view(U32)[:] = 0
        p.update(cancel_step=1, cancel_slot=slots[0])             # the first row's slot has emitted once when its request goes away, in front of step 1
        w = np.zeros(1, WATCH_DT)
        w["ring"], w["cancel"], w["ring_steps"] = 0, ring_steps * rec_bytes(B) + 16, ring_steps
        W["watch"], W["ring"] = w, ring
    p.update(any_miro=int((s["kind"] == 2).any()))

    def image(i, W):
        g = rng_of(f"{name}/{i}")
        x = np.full((n, V), -INF, F32)
        for r, slot in enumerate(slots):
            ids = np.arange(1, V)
            bad = np.zeros(0, np.int64)
            if "dfa" in W and W["dfa"][slot]["trans"] != -1:
                e = dfa_ends(W["dfa_trans"].reshape(-1, 256), int(W["dfa"][slot]["state"]), W["tok_off"], W["tok_bytes"], p["n_tok"], V)
                ids, bad = np.nonzero(e)[0], np.nonzero(e == 0)[0][:5]
            if "pda" in W and W["pda"][slot]["next"] != -1:
                d = W["pda"][slot]
                nxt, act, _ = pda_tables(W, p, d)
                ok = np.array([bool(v) and bool(token_word(W, p, v)) and bool(pda_walk(nxt, act, int(d["max_depth"]), int(d["state"]),
                               [int(z) for z in d["stack"][:int(d["depth"])]], token_word(W, p, v))[0]) for v in range(V)])
                ids, bad = np.nonzero(ok)[0], np.nonzero(~ok)[0][:5]
            assert ids.size >= 2, (name, i, r)
            live = g.choice(ids, 1 << min(3, int(np.log2(ids.size))), replace=False)
            sl = W["slots"][slot]
            for t in np.concatenate([live, bad]):
                pb = W["penalty"][slot].view(U32)[t]
                b = W["bias"][slot][t] if sl["has_bias"] else F32(0)
                edit = F32(0)
                if not sl["finish"]:                               # a rider's row is sampled as it stands
                    if sl["kind"] != 2 and pb != ABSENT:
                        edit = F32(F32(-W["penalty"][slot][t]) + b) if b != 0 else F32(-W["penalty"][slot][t])
                    elif b != 0:
                        edit = b
                x[r, t] = F32(1.5) - edit
        return x
    if scene == "penalties_bias_stop":                             # a dry run finds the token the first row draws in step 1: it becomes a stop token
        dry = copy.deepcopy(W)
        ref_step(dry, p, image=image)
        s["n_stop"][slots[0]] = 8
        s["stop"][slots[0]] = [70000 + j for j in range(7)] + [int(dry["out_tok"][1 * B + slots[0]])]
    ref_step(copy.deepcopy(W), p, image=lambda i, Wc: _store(W, i, image(i, Wc), n, V))
    return W, p


def _store(W, i, x, n, V):
    W["logits_steps"][i * n * V:(i + 1) * n * V] = x.reshape(-1)
    return x


def topn_world(name, V, B, mixed, n, run_step, pair):
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=run_step)
    p.update(steps=6, n=n)
    R = TN.rows_of(V)
    names = ["normal0", "tie40", "zeros", "dyadic3", "alt_inf"]
    W["logits"] = np.stack([R[names[(r + n) % len(names)]] for r in range(p["n_rows"])])
    tn = np.full(B, n, I32)
    if B > 1:
        tn[row_slots(W, p)[-1]] = 0                                # a slot that lists nothing
    W["topn_n"] = tn
    W["top_ids"], W["top_logp"] = sent(6 * B * TOPN_MAX), sent(6 * B * TOPN_MAX).view(F32)
    W["side_ms"], W["side_rows"] = sent(p["n_rows"] * 2).view(F32), sent(p["n_rows"] * V).view(F32)
    if pair:
        W["out_ids2"], W["out_logp2"] = sent(p["n_rows"] * n), sent(p["n_rows"] * n).view(F32)
        W["side_ms2"], W["side_rows2"] = sent(p["n_rows"] * 2).view(F32), sent(p["n_rows"] * V).view(F32)
    return W, p


def state_world(name, kind, V, B, mixed, nsx, nw, var):
    W, rng, p, riders = base_world(name, V, B, mixed, run_step=3)
    p.update(nsx=nsx, nw=nw)
    slots = row_slots(W, p)
    W["sxa"], W["sxf"], W["wkv"] = (rng.standard_normal(B * n).astype(F32) for n in (nsx, nsx, nw))
    item = 2 * nsx + nw
    if kind == "gen_freeze":
        sh = np.full(B, -1, np.int64)
        W["shadow_mem"] = sent(B * item + 64).view(F32)
        for r, slot in enumerate(slots):
            g = W["slots"][slot]
            mode = (r + var) % 4                                   # 0 copies; 1 finished in another step; 2 still running; 3 finished now, null shadow
            g["finish"], g["freeze_at"] = (1, 3) if mode in (0, 3) else (2, 2) if mode == 1 else (0, 3)
            if slot in riders:
                g["finish"], g["freeze_at"] = 1, 1
            sh[slot] = -1 if mode == 3 else slot * item + 64
        W["shadow"] = sh
        return W, p
    W["logits"] = logits_rows(rng, p["n_rows"], V)
    cap = np.full(B, -1, np.int64).repeat(4).reshape(B, 4).copy().view(CAP_DT).reshape(B)
    if kind == "gen_inject":
        p.update(first_row=var % p["n_rows"])
        W["cap_mem"] = rng.standard_normal(B * V + 16).astype(F32)
        for r, slot in enumerate(slots):
            if r != p["first_row"] or p["n_rows"] - p["first_row"] == 1 or var % 2 == 0:   # one row past first_row may have no item: it keeps its row
                cap[slot]["inj_row"] = slot * V + 16
        W["cap"] = cap
        return W, p
    W["cap_mem"] = sent(B * (item + 2 * V)).view(F32)
    for r, slot in enumerate(slots):
        mode = (r + var) % 4                                       # 0 f_row only; 1 p_row only, draws == 0; 2 both; 3 p_row with draws > 0 and f_row
        at = slot * (item + 2 * V)
        if slot in riders:
            mode = 2                                               # a rider that asks for both writes nothing
        if mode in (0, 2, 3):
            cap[slot]["f_row"] = at + item + V
        if mode in (1, 2, 3):
            cap[slot]["p_state"], cap[slot]["p_row"] = at, at + item
        W["slots"][slot]["draws"] = 5 if mode == 3 else 0
    W["cap"] = cap
    return W, p


def publish_world(name, B, var):
    """var: 0 plain; 1 run_step -1 (padding); 2 cancel words; 3 seq = ring_steps - 1; 4 seq = ring_steps (the wrap); 5 null ring."""
    rng = rng_of(name)
    steps, ring_steps = 5, 4
    run_step = -1 if var == 1 else 3
    s = np.zeros(B, SLOT_DT)
    s["freeze_at"] = -1
    s["finish"] = [(0, 0, 1, 0, 2)[b % 5] for b in range(B)]
    W = {"slots": s, "run_step": np.array([run_step], I32)}
    out_tok = rng.integers(1, 60000, steps * B).astype(U32)
    out_tok[np.arange(steps * B) % B % 4 == 3] = NO_TOKEN          # slots that did not draw in a step
    W["out_tok"], W["out_prob"] = out_tok, rng.uniform(0.1, 1.0, steps * B).astype(F32)
    ring = np.full(ring_bytes(ring_steps, B), 0xAD, U8)
    cancel = ring[ring_steps * rec_bytes(B) + 16:].view(U32)
    cancel[:] = 0
    if var == 2:
        cancel[:] = [1 if b % 2 == 0 or b % 4 == 3 else 0 for b in range(B)]   # running slots that drew, slots that did not draw, finished ones
        if B >= 3:
            cancel[2] = 1
    ring[ring_steps * rec_bytes(B):][:8].view(np.uint64)[0] = 0
    w = np.zeros(1, WATCH_DT)
    w["ring"], w["cancel"], w["ring_steps"] = (-1, -1, ring_steps) if var == 5 else (0, ring_steps * rec_bytes(B) + 16, ring_steps)
    w["seq"] = {3: ring_steps - 1, 4: ring_steps}.get(var, 1)
    W["watch"], W["ring"] = w, ring
    return W, params(V=16, max_batch=B, steps=steps, ring_steps=ring_steps)


def tokens_world(name, kind, T, to_held):
    rng = rng_of(name)
    B = 5
    W = {"row_slot": rng.integers(0, B, max(T, 1)).astype(I32), "held": rng.integers(1, 60000, B).astype(I32), "run_step": np.array([4], I32)}
    if kind == "gen_tokens":
        tok = rng.integers(0, 60000, max(T, 1)).astype(I32)
        tok[::3] = -1
        if T > 1:
            tok[T - 1] = -1
        W["token"] = tok
    else:
        W["feedback"] = rng.integers(1, 60000, T).astype(I32)
        if to_held:                                                # rows of distinct slots, as a decode-only step has them
            W["row_slot"] = np.arange(T, dtype=I32)
            W["held"] = rng.integers(1, 60000, T).astype(I32)
            B = T
    return W, params(V=16, max_batch=B, T=T, to_held=int(to_held))


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
_ALL = []


def _case(name, group, kind, fn, *args, **tags):
    """The table keeps a small world (a copy is handed out); a large one is made anew whenever it is asked for — every generator is seeded
    by the case's name, and the large ones are plain numpy fills."""
    W, p = fn(name, *args)
    small = sum(a.nbytes for a in W.values()) <= 1 << 20
    return Case(name, group, KIND[kind], p, {"world": (lambda: copy.deepcopy(W)) if small else (lambda: fn(name, *args)[0]), "tags": tags})


def all_cases():
    if _ALL:
        return _ALL
    cs = []
    combos = {16: [(1, 0), (3, 0), (5, 0), (1, 1), (3, 1), (5, 1)], 1024: [(3, 0), (3, 1)], 16384: [(5, 0), (1, 1)], 16400: [(1, 0), (3, 0), (5, 0), (1, 1), (3, 1), (5, 1)],
              65536: [(3, 0), (5, 1)]}
    j = 0
    for V in VOCABS:
        for B, mixed in combos[V]:
            cs.append(_case(f"pre_V{V}_B{B}_m{mixed}", "pre", "gen_pre", pre_world, V, B, mixed, j % 3, V=V, B=B, mixed=mixed))
            cs.append(_case(f"post_V{V}_B{B}_m{mixed}", "post", "gen_post", post_world, V, B, mixed, j, V=V, B=B, mixed=mixed))
            j += 1
    for V in VOCABS:                                               # the drawn token of a LIVE row at every place of POST_TOKS that the row has, and at V - 1
        at = [t for t in POST_TOKS + (V - 1,) if t < V]
        for j in range(0, len(at), 2):
            cs.append(_case(f"post_V{V}_at{at[j]}", "post", "gen_post", post_world, V, 3, j // 2 % 2, j, False, False, False, (at + at)[j:j + 2], V=V, B=3, mixed=j // 2 % 2,
                            at=(at + at)[j:j + 2]))
    for j, (V, B, mixed) in enumerate([(1024, 5, 0), (16400, 3, 1), (65536, 5, 1), (16, 5, 0)]):
        cs.append(_case(f"post_dfa_V{V}_B{B}_m{mixed}", "post", "gen_post", post_world, V, B, mixed, j, True, False, V=V, B=B, mixed=mixed, dfa=1))
        cs.append(_case(f"post_topn_V{V}_B{B}_m{mixed}", "post", "gen_post", post_world, V, B, mixed, j, False, True, V=V, B=B, mixed=mixed, topn=1))
    for j in range(5):
        B, mixed = (5, 3)[j % 2], j % 2
        cs.append(_case(f"post_pda_{j}", "post", "gen_post", post_world, 1024, B, mixed, j, False, False, True, V=1024, B=B, mixed=mixed, pda=1))
    names = list(STOP_SCENES)
    for j in range(0, len(names), 2):                              # every scene in a decode-only launch and in a mixed one, at different rows
        for mixed in (0, 1):
            sc = [names[j], names[(j + 7) % len(names)], names[j + 1]]   # rows 0 and 2 are live, row 1 is the rider
            if mixed:
                sc = sc[::-1]
            cs.append(_case(f"stops_{j // 2}_m{mixed}", "stops", "gen_post", stops_world, 1024, 5, mixed, sc, scenes=names[j:j + 2], mixed=mixed))
    cs.append(_case("stops_B1", "stops", "gen_post", stops_world, 16400, 1, 0, ["string7_alone"], scenes=["string7_alone"], mixed=0))
    for V in MASK_VOCABS:
        for j, (B, mixed, full) in enumerate([(5, 0, 1), (3, 1, 0), (5, 1, 1), (1, 0, 0)]):
            n_tok = V if full else V - 3
            cs.append(_case(f"mask_V{V}_B{B}_m{mixed}_n{n_tok}", "mask", "gen_mask", mask_world, V, B, mixed, n_tok, V=V, B=B, mixed=mixed, n_tok=n_tok))
    deep = [1, 2] * 32                                             # 64 entries, the two return states alternating: entry 63 is 2, entry 31 is 2, entry 32 is 1
    # depth 0 and 64 (a pop takes entry 63) | max_depth 6 reached in mid-token beside an unconstrained slot | depth 63 and 3 (row 1 of five slots is the rider)
    bracket = [[(1, [], 64, 0), None, (1, deep, 64, 1)], [(2, deep[:5], 6, 0), None], [(1, deep[:63], 64, 0), None, (1, deep[:3], 64, 0)]]
    for V in MASK_VOCABS:
        for j, (B, mixed) in enumerate([(5, 0), (3, 1), (5, 1)]):
            cfg = bracket[j]
            cs.append(_case(f"pda_bracket_V{V}_B{B}_m{mixed}", "pda", "gen_pda_mask", pda_world, V, B, mixed, V - (j % 2) * 3, "bracket", cfg, V=V, B=B, mixed=mixed, table="bracket"))
    for j, text in enumerate([b"", b'{"a": [1, {"b": ', b'[[[[']):
        cs.append(_case(f"pda_json_{j}", "pda", "gen_pda_mask", lambda name, t=text, j=j: pda_world(name, 272, 3, j % 2, 272, "json", [json_config(t, 64 if j < 2 else 5), None]),
                        V=272, B=3, mixed=j % 2, table="json"))
    for V in (16, 272, 65536):
        for n, B, mixed, rs in [(1, 5, 0, -1), (32, 3, 0, 3), (32, 5, 1, 0), (1, 3, 1, 3), (5, 1, 0, 3)]:
            for pair in (0, 1):
                cs.append(_case(f"topn{'_pair' if pair else ''}_V{V}_n{n}_B{B}_m{mixed}_k{rs}", "topn", "topn_pair" if pair else "gen_topn", topn_world, V, B, mixed, n, rs, pair,
                                V=V, n=n, B=B, mixed=mixed, run_step=rs))
    j = 0
    for nsx in SX_STRIDES:
        for nw in WKV_STRIDES:
            for B, mixed in [(5, 0), (3, 1), (5, 1), (1, 0)]:
                if (nsx, nw) != (65600, 131136) or B == 5:
                    cs.append(_case(f"freeze_sx{nsx}_w{nw}_B{B}_m{mixed}", "state", "gen_freeze", state_world, "gen_freeze", 16, B, mixed, nsx, nw, j, nsx=nsx, nw=nw, B=B, mixed=mixed))
                    cs.append(_case(f"capture_sx{nsx}_w{nw}_B{B}_m{mixed}", "state", "gen_capture", state_world, "gen_capture", (16, 1024)[j % 2], B, mixed, nsx, nw, j, nsx=nsx, nw=nw,
                                    B=B, mixed=mixed))
                    j += 1
    for j, V in enumerate(VOCABS):
        for B in (5, 3) if V in (16, 16400) else (5,):
            cs.append(_case(f"inject_V{V}_B{B}", "state", "gen_inject", state_world, "gen_inject", V, B, 1, 64, 64, j + B, V=V, B=B, mixed=1))
    for mixed in (0, 1):                                           # the wide worlds: 72 slots, 33 logits rows decode-only, 34 of 70 step rows mixed
        B = WIDE_B
        cs.append(_case(f"pre_V1024_B{B}_m{mixed}", "pre", "gen_pre", pre_world, 1024, B, mixed, 2 * mixed, V=1024, B=B, mixed=mixed))
        cs.append(_case(f"post_V1024_B{B}_m{mixed}", "post", "gen_post", post_world, 1024, B, mixed, 3 + mixed, V=1024, B=B, mixed=mixed))
        cs.append(_case(f"mask_V272_B{B}_m{mixed}_n272", "mask", "gen_mask", mask_world, 272, B, mixed, 272, V=272, B=B, mixed=mixed, n_tok=272))
        cs.append(_case(f"freeze_sx64_w64_B{B}_m{mixed}", "state", "gen_freeze", state_world, "gen_freeze", 16, B, mixed, 64, 64, mixed, nsx=64, nw=64, B=B, mixed=mixed))
        cs.append(_case(f"capture_sx64_w64_B{B}_m{mixed}", "state", "gen_capture", state_world, "gen_capture", 16, B, mixed, 64, 64, 1 + mixed, nsx=64, nw=64, B=B, mixed=mixed))
    for B in (1, 3, 257):
        for var in range(6):
            cs.append(_case(f"publish_B{B}_v{var}", "publish", "gen_publish", publish_world, B, var, B=B, var=var))
    for T in TOKEN_ROWS:
        cs.append(_case(f"tokens_T{T}", "tokens", "gen_tokens", tokens_world, "gen_tokens", T, 0, T=T))
        if T:
            for to_held in (0, 1):
                cs.append(_case(f"handover_T{T}_h{to_held}", "tokens", "gen_handover", tokens_world, "gen_handover", T, to_held, T=T, to_held=to_held))
    for sc in STEP_SCENES:
        cs.append(_case(f"step_{sc}", "step", "step", step_world, sc, scene=sc))
    assert len({c.name for c in cs}) == len(cs)
    _ALL.extend(cs)
    return _ALL


# ------------------------------------------------------------------------------------------------
# coverage, from the table alone
# ------------------------------------------------------------------------------------------------
def coverage(cases):
    got = set()
    for c in cases:
        k, t = KIND_NAME[c.kind], c.o["tags"]
        got.add(f"kind:{k}")
        got.add(f"{k}:B{c.p['max_batch']}")
        got.add(f"{k}:mixed{c.p['mixed']}")
        if k in ("gen_pre", "gen_post", "gen_inject", "gen_mask", "gen_pda_mask", "gen_topn", "topn_pair"):
            got.add(f"{k}:V{c.p['V']}")
        if k in ("gen_freeze", "gen_capture"):
            got.add(f"{k}:nsx{c.p['nsx']}")
            got.add(f"{k}:nw{c.p['nw']}")
        if k == "gen_publish":
            got.add(f"publish:var{t['var']}")
        if k in ("gen_tokens", "gen_handover"):
            got.add(f"{k}:T{c.p['T']}")
        for s in t.get("scenes", ()):
            got.add(f"stops:{s}:mixed{c.p['mixed']}")
        for x in ("dfa", "topn", "pda"):
            if t.get(x):
                got.add(f"gen_post:{x}")
        if "scene" in t:
            got.add(f"step:{t['scene']}")
        if "table" in t:
            got.add(f"gen_pda_mask:{t['table']}")
    return got


WANTED = ([f"kind:{k}" for k in KIND_NAME] + [f"{k}:V{V}" for k in ("gen_pre", "gen_post", "gen_inject") for V in VOCABS]
          + [f"{k}:V{V}" for k in ("gen_mask", "gen_pda_mask") for V in MASK_VOCABS] + [f"{k}:V{V}" for k in ("gen_topn", "topn_pair") for V in (16, 272, 65536)]
          + [f"{k}:B{B}" for k in ("gen_pre", "gen_post", "gen_mask", "gen_freeze", "gen_capture") for B in (1, 3, 5, WIDE_B)] + [f"gen_publish:B{B}" for B in (1, 3, 257)]
          + [f"{k}:mixed{m}" for k in ("gen_pre", "gen_post", "gen_mask", "gen_pda_mask", "gen_topn", "gen_freeze", "gen_capture") for m in (0, 1)]
          + [f"{k}:nsx{n}" for k in ("gen_freeze", "gen_capture") for n in SX_STRIDES] + [f"{k}:nw{n}" for k in ("gen_freeze", "gen_capture") for n in WKV_STRIDES]
          + [f"publish:var{v}" for v in range(6)] + [f"gen_tokens:T{T}" for T in TOKEN_ROWS] + [f"gen_handover:T{T}" for T in TOKEN_ROWS if T]
          + [f"stops:{s}:mixed{m}" for s in STOP_SCENES for m in (0, 1)] 
          + ["gen_post:dfa", "gen_post:topn", "gen_post:pda", "gen_pda_mask:bracket", "gen_pda_mask:json"] + [f"step:{s}" for s in STEP_SCENES])


def coverage_gaps(cases):
    got = coverage(cases)
    return [w for w in WANTED if w not in got]
