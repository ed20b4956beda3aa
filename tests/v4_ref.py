"""The checker of the RWKV-4 path: a numpy evaluation of the V4 forward pass, float64 unless asked otherwise.

Per layer, on the ln1 row `xx` with `sx` the previous row of the slot (or the state):

    xk = xx*mu_k + sx*(1-mu_k)   (likewise xv, xr);   r = sigmoid(Wr xr), k = Wk xk, v = Wv xv
    per channel, u = time_first, w = -exp(time_decay):
        ww = u + k;  p = max(pp, ww);  e1 = exp(pp - p);  e2 = exp(ww - p);  wkv = (e1*aa + e2*v) / (e1*bb + e2)
        ww = pp + w; p = max(ww, k);   e1 = exp(ww - p);  e2 = exp(k - p);   aa = e1*aa + e2*v;  bb = e1*bb + e2;  pp = p
    x += Wo (r * wkv);   channel mix as V5: x += sigmoid(Fr xr) * Fv relu(Fk xk)^2

Weights are read through fp16, as the `.st` stores them; matrices of quantised layers go through `oracle.rwkv_ref.fake_quant`.
State: [5L][C], layer l owns rows 5l .. 5l+4 = att shift, aa, bb, pp, ffn shift; the initial state is 0 with -1e30 in the pp rows."""
import re
from types import SimpleNamespace

import numpy as np

from oracle import rwkv_ref as R

CONFIGS = {"v4-tiny": (4, 2, 128, 512, 512), "v4-small": (4, 3, 256, 1024, 1024)}   # version, L, C, F, V
QUANT_NAMES = ["att.receptance.weight", "att.key.weight", "att.value.weight", "att.output.weight",
               "ffn.key.weight", "ffn.value.weight", "ffn.receptance.weight"]
PP_INIT = -1e30
LN_EPS = 1e-5
GREEDY_RUN = (40, 9, 96)               # prompt slot number, prompt length, steps of the greedy run (tests/test_gpu_v4.py; its CPU screen: tests/test_v4_cpu.py)


def synth_checkpoint_v4(L, C, F, V, seed=20251024):
    """Seeded fp16 tensors with the names and shapes of a converted V4 `.st` (the converter renames and transposes nothing for V4):
    matrices N(0, (0.5/sqrt(in))^2), time_decay uniform[-6, -0.5], time_first N(0, 0.3^2), mixes uniform[0, 1]."""
    rng = np.random.Generator(np.random.SFC64(seed))
    t = {}
    f16 = lambda a: np.asarray(a, np.float32).astype(np.float16)
    mat = lambda o, i, std=None: f16(rng.standard_normal((o, i), dtype=np.float32) * np.float32(0.5 / np.sqrt(i) if std is None else std))
    vec = lambda mean=0.0, std=0.02: f16(mean + rng.standard_normal(C, dtype=np.float32) * np.float32(std))
    t["emb.weight"] = mat(V, C, 0.5)
    for l in range(L):
        p = f"blocks.{l}."
        if l == 0:
            t[p + "ln0.weight"], t[p + "ln0.bias"] = vec(1.0), vec()
        for ln in ("ln1", "ln2"):
            t[p + ln + ".weight"], t[p + ln + ".bias"] = vec(1.0), vec()
        for n in "kvr":
            t[p + f"att.time_mix_{n}"] = f16(rng.uniform(0, 1, size=(1, 1, C)))
        t[p + "att.time_decay"] = f16(rng.uniform(-6, -0.5, size=C))
        t[p + "att.time_first"] = vec(0.0, 0.3)
        for n in ("receptance", "key", "value", "output"):
            t[p + f"att.{n}.weight"] = mat(C, C)
        for n in "kr":
            t[p + f"ffn.time_mix_{n}"] = f16(rng.uniform(0, 1, size=(1, 1, C)))
        t[p + "ffn.receptance.weight"] = mat(C, C)
        t[p + "ffn.key.weight"] = mat(F, C)
        t[p + "ffn.value.weight"] = mat(C, F)
    t["ln_out.weight"], t["ln_out.bias"] = vec(1.0), vec()
    t["head.weight"] = mat(V, C)
    return t


def synth_v4(name, seed=20251024):
    _, L, C, F, V = CONFIGS[name]
    return synth_checkpoint_v4(L, C, F, V, seed)


def blend_lora(tensors, lora, alpha):
    """`LoraBlend::full(alpha)` on the matrices of `blocks.N.*`: W += alpha * B A^T with `X.lora.0` = A [in, r] and `X.lora.1` = B [out, r],
    in fp32 on the fp16 values and rounded back to fp16 once, before any quantisation (oracle/rwkv_ref.py RwkvRef does the same).
    Any other tensor of a block that the file holds under the model's own name (`time_decay`, `time_first`, a mix vector) is blended
    whole, v = alpha * l + (1 - alpha) * v in fp32 on the fp16 values, and STAYS fp32 (the loader blends first and transforms after:
    V4's -exp(time_decay) is taken of the blend); V4Ref reads a float32 tensor as it is."""
    out = dict(tensors)
    for k, v in tensors.items():
        if not re.fullmatch(r"blocks\.[0-9]+\..+", k):
            continue
        stem = k[:-len(".weight")] if k.endswith(".weight") else k
        if stem + ".lora.0" in lora and np.ndim(v) == 2:
            A = np.asarray(lora[stem + ".lora.0"], np.float16).astype(np.float32)
            B = np.asarray(lora[stem + ".lora.1"], np.float16).astype(np.float32)
            out[k] = (np.asarray(v, np.float16).astype(np.float32) + np.float32(alpha) * (B @ A.T)).astype(np.float16)
        elif k in lora:
            base = np.asarray(v, np.float16).astype(np.float32)
            out[k] = np.float32(alpha) * np.asarray(lora[k], np.float16).astype(np.float32).reshape(base.shape) + (np.float32(1.0) - np.float32(alpha)) * base
    return out


class _RowSums(np.ndarray):
    """A matrix whose product with a vector is numpy's own pairwise sum of every row instead of the BLAS's (`V4Ref(pairwise_sums=True)`)."""

    def __matmul__(self, x):
        return (np.asarray(self) * np.asarray(x)).sum(axis=1)


class V4Ref:
    """`clip_operands`: every activation a matrix multiplies is clamped to +-65504 first, the engine's saturation contract as
    `oracle.rwkv_ref.RwkvRef` states it.  `round_operands`: names of the launch classes (OPERAND_CLASSES) whose activation operand is rounded
    to f16 on the way in, after the clamp: what Precision::Fp16 does to every class it does not promote (V4: all but `att`, FP16_PLAIN).
    `self.probe`, when set to a callable `(name, layer, array)`, is shown, in this order per layer, `emb_row` (layer -1), `wdec` (the per-channel w), `k`,
    `pp_step` (pp and pp + w), `e_state` (the two e1 of a token: row 0 the output half's, row 1 the state update's), `wkv_out` and `relu2` (the
    operand of ffn.value).  `pairwise_sums`: matrix-vector products are numpy's pairwise row sums, so that a float32 evaluation gives the
    same figures whichever kernel the BLAS picks for a CPU.  All four are off by default and then touch nothing."""
    OPERAND_CLASSES = ("att", "wo", "ffn1", "fv", "head")
    FP16_PLAIN = ("wo", "ffn1", "fv", "head")                       # promote_for_version(4) promotes CLS_ATT only

    def __init__(self, tensors, quant_layers=0, quant_type=R.QUANT_NONE, dtype=np.float64, clip_operands=False, round_operands=(),
                 pairwise_sums=False):
        assert set(round_operands) <= set(self.OPERAND_CLASSES), round_operands
        self.dt = dtype
        self.clip_operands, self.round_operands, self.probe = clip_operands, tuple(round_operands), None
        L = sum(1 for k in tensors if k.endswith(".ln1.weight"))
        V, C = tensors["emb.weight"].shape
        F = tensors["blocks.0.ffn.key.weight"].shape[0]
        self.info = SimpleNamespace(version=4, num_layer=L, num_emb=C, num_hidden=F, num_vocab=V, num_head=1, head_size=C)
        qn = {f"blocks.{l}.{n}" for l in range(min(quant_layers, L)) for n in QUANT_NAMES} if quant_type != R.QUANT_NONE else set()
        self.w = {}
        for k, v in tensors.items():
            if np.asarray(v).dtype == np.float32 and np.squeeze(v).ndim == 1:   # a vector `blend_lora` blended: fp32, as the loader keeps it
                v16 = np.asarray(v)
            else:
                v16 = np.asarray(v, np.float16)
            if k in qn:
                v16 = R.fake_quant(v16, quant_type)
            a = v16.astype(dtype)
            self.w[k] = (a.view(_RowSums) if pairwise_sums and k != "emb.weight" else a) if a.ndim == 2 else a.reshape(-1)
        self.k_absmax = 0.0                                          # largest |k| any token has produced so far (what the range test aims at)

    def init_state(self):
        i = self.info
        s = np.zeros((5 * i.num_layer, i.num_emb), self.dt)
        s[3::5] = PP_INIT
        return s

    def _ln(self, x, w, b):
        m = x.mean()
        v = ((x - m) ** 2).mean()
        return (x - m) / np.sqrt(v + self.dt(LN_EPS)) * w + b

    def _sigmoid(self, x):
        with np.errstate(over="ignore"):                            # exp(-x) = inf gives the exact 0 it should
            return self.dt(1) / (self.dt(1) + np.exp(-x))

    def _opd(self, x, cls):
        """A GEMM's activation operand of launch class `cls` (see `clip_operands`, `round_operands`)."""
        if self.clip_operands:
            x = np.clip(x, self.dt(-65504.0), self.dt(65504.0))
        if cls in self.round_operands:
            x = x.astype(np.float16).astype(self.dt)
        return x

    def _show(self, name, layer, a):
        if self.probe is not None:
            self.probe(name, layer, a)

    def _token(self, token, s, want_logits=True):
        w = self.w
        self._show("emb_row", -1, w["emb.weight"][token])
        x = self._ln(w["emb.weight"][token], w["blocks.0.ln0.weight"], w["blocks.0.ln0.bias"])
        for l in range(self.info.num_layer):
            p, a, f = f"blocks.{l}.", f"blocks.{l}.att.", f"blocks.{l}.ffn."
            xx = self._ln(x, w[p + "ln1.weight"], w[p + "ln1.bias"])
            sx = s[5 * l].copy()
            s[5 * l] = xx
            mix = lambda mu: self._opd(xx * mu + sx * (1 - mu), "att")
            r = self._sigmoid(w[a + "receptance.weight"] @ mix(w[a + "time_mix_r"]))
            k = w[a + "key.weight"] @ mix(w[a + "time_mix_k"])
            v = w[a + "value.weight"] @ mix(w[a + "time_mix_v"])
            self.k_absmax = max(self.k_absmax, float(np.abs(k).max()))
            aa, bb, pp = s[5 * l + 1], s[5 * l + 2], s[5 * l + 3]
            u, wd = w[a + "time_first"], -np.exp(w[a + "time_decay"])
            ww = u + k
            q = np.maximum(pp, ww)
            e1, e2 = np.exp(pp - q), np.exp(ww - q)
            wkv = (e1 * aa + e2 * v) / (e1 * bb + e2)
            e_out = e1
            ww = pp + wd
            q = np.maximum(ww, k)
            e1, e2 = np.exp(ww - q), np.exp(k - q)
            if self.probe is not None:
                for name, arr in (("wdec", wd), ("k", k), ("pp_step", np.stack([pp, ww])), ("e_state", np.stack([e_out, e1])), ("wkv_out", wkv)):
                    self.probe(name, l, arr)
            s[5 * l + 1], s[5 * l + 2], s[5 * l + 3] = e1 * aa + e2 * v, e1 * bb + e2, q
            x = x + w[a + "output.weight"] @ self._opd(r * wkv, "wo")
            xx = self._ln(x, w[p + "ln2.weight"], w[p + "ln2.bias"])
            sx = s[5 * l + 4].copy()
            s[5 * l + 4] = xx
            mix = lambda mu: self._opd(xx * mu + sx * (1 - mu), "ffn1")
            kk = np.maximum(w[f + "key.weight"] @ mix(w[f + "time_mix_k"]), 0) ** 2
            self._show("relu2", l, kk)
            x = x + self._sigmoid(w[f + "receptance.weight"] @ mix(w[f + "time_mix_r"])) * (w[f + "value.weight"] @ self._opd(kk, "fv"))
        if not want_logits:
            return None
        return w["head.weight"] @ self._opd(self._ln(x, w["ln_out.weight"], w["ln_out.bias"]), "head")

    def forward(self, tokens, state, full=False):
        """Consume `tokens` in order, `state` [5L][C] is updated in place.  Returns the logits of the last token [1, V], or with `full` one
        row per token."""
        rows = []
        for t, tok in enumerate(tokens):
            want = full or t == len(tokens) - 1
            lg = self._token(int(tok), state, want)
            if want:
                rows.append(lg)
        return np.stack(rows) if rows else np.zeros((0, self.info.num_vocab), self.dt)

    def greedy(self, prompt, n_new, state=None):
        state = self.init_state() if state is None else state
        lg = self.forward(list(prompt), state)[-1]
        out = []
        for _ in range(n_new):
            t = int(np.argmax(lg))
            out.append(t)
            lg = self.forward([t], state)[-1]
        return out, state


def prompt(V, slot, n):
    """`n` token ids in [1, V) for slot number `slot` (oracle.rwkv_ref.synth_prompt folded into the vocabulary, 0 avoided: it stops a decode loop)"""
    return [1 + t % (V - 1) for t in R.synth_prompt(slot, n)]
