"""Second, independent form of the RWKV-4 forward pass: BlinkDL's PUBLISHED single-token `RWKV_RNN` functions (`RWKV_in_150_lines.py`:
`layer_norm`, `channel_mixing`, `time_mixing`, `forward`), restated with torch in the ORIGINAL layout of that script — the `.pth` tensors as
the trainer saves them, `time_decay` turned into `-exp(time_decay)` at load, and the state as ONE [5L][C] tensor whose rows per layer are

    5i+0  channel-mix shift     5i+1  time-mix shift     5i+2  aa     5i+3  bb     5i+4  pp  (initialised to -1e30)

which is NOT the row order of the engine's slab (att shift, aa, bb, pp, ffn shift): `to_slab_order` maps one onto the other.  Test-only: it
pins tests/v4_ref.py, and through it the engine, against a form that keeps its state differently."""
import numpy as np
import torch
import torch.nn.functional as F

SLAB_ROW_OF = [4, 0, 1, 2, 3]          # literal row j of a layer is slab row SLAB_ROW_OF[j]


class LiteralV4:
    def __init__(self, pth: dict, dtype=torch.float64):
        w = {}
        for k, a in pth.items():
            t = torch.from_numpy(np.asarray(a, np.float16).astype(np.float64)).to(dtype)
            if ".time_" in k:
                t = t.squeeze()
            if ".time_decay" in k:
                t = -torch.exp(t)
            w[k] = t
        self.w, self.dtype = w, dtype
        self.L = sum(1 for k in pth if k.endswith(".ln1.weight"))
        self.C = pth["emb.weight"].shape[1]

    def new_state(self):
        s = torch.zeros(5 * self.L, self.C, dtype=self.dtype)
        for i in range(self.L):
            s[5 * i + 4] = -1e30
        return s

    def layer_norm(self, x, p):
        return F.layer_norm(x, (self.C,), weight=self.w[p + ".weight"], bias=self.w[p + ".bias"])

    def channel_mixing(self, x, state, i, time_mix_k, time_mix_r, kw, vw, rw):
        xk = x * time_mix_k + state[5 * i + 0] * (1 - time_mix_k)
        xr = x * time_mix_r + state[5 * i + 0] * (1 - time_mix_r)
        state[5 * i + 0] = x
        r = torch.sigmoid(rw @ xr)
        k = torch.square(torch.relu(kw @ xk))
        return r * (vw @ k)

    def time_mixing(self, x, state, i, time_mix_k, time_mix_v, time_mix_r, time_first, time_decay, kw, vw, rw, ow):
        xk = x * time_mix_k + state[5 * i + 1] * (1 - time_mix_k)
        xv = x * time_mix_v + state[5 * i + 1] * (1 - time_mix_v)
        xr = x * time_mix_r + state[5 * i + 1] * (1 - time_mix_r)
        state[5 * i + 1] = x
        r = torch.sigmoid(rw @ xr)
        k = kw @ xk
        v = vw @ xv
        aa, bb, pp = state[5 * i + 2], state[5 * i + 3], state[5 * i + 4]
        ww = time_first + k
        qq = torch.maximum(pp, ww)
        e1, e2 = torch.exp(pp - qq), torch.exp(ww - qq)
        a = e1 * aa + e2 * v
        b = e1 * bb + e2
        wkv = a / b
        ww = pp + time_decay
        qq = torch.maximum(ww, k)
        e1, e2 = torch.exp(ww - qq), torch.exp(k - qq)
        state[5 * i + 2] = e1 * aa + e2 * v
        state[5 * i + 3] = e1 * bb + e2
        state[5 * i + 4] = qq
        return ow @ (r * wkv)

    def forward(self, token, state):
        w = self.w
        x = self.layer_norm(w["emb.weight"][token], "blocks.0.ln0")
        for i in range(self.L):
            a, f = f"blocks.{i}.att.", f"blocks.{i}.ffn."
            x = x + self.time_mixing(self.layer_norm(x, f"blocks.{i}.ln1"), state, i, w[a + "time_mix_k"], w[a + "time_mix_v"], w[a + "time_mix_r"],
                                     w[a + "time_first"], w[a + "time_decay"], w[a + "key.weight"], w[a + "value.weight"],
                                     w[a + "receptance.weight"], w[a + "output.weight"])
            x = x + self.channel_mixing(self.layer_norm(x, f"blocks.{i}.ln2"), state, i, w[f + "time_mix_k"], w[f + "time_mix_r"],
                                        w[f + "key.weight"], w[f + "value.weight"], w[f + "receptance.weight"])
        return (w["head.weight"] @ self.layer_norm(x, "ln_out")).numpy()

    def to_slab_order(self, state):
        """the literal's state as the engine's slab [5L][C] orders it"""
        s = state.numpy()
        out = np.empty_like(s)
        for i in range(self.L):
            for j in range(5):
                out[5 * i + SLAB_ROW_OF[j]] = s[5 * i + j]
        return out
