"""Host-side mirror of the `web-rwkv` surface that ai00-core uses, bound to librwkv_hip.so over ctypes.

Names follow the reference imports (crates/ai00-core/src/lib.rs:24-35, run.rs:22-31):

    Loader.info            lib.rs:587            -> ModelInfo
    ModelBuilder(...).quant(..).lora(..).build() lib.rs:484-516  -> Runtime (+ .state)
    Runtime.infer(RnnInput) -> (RnnInput, RnnOutput)   run.rs:1143
    RnnInput / RnnInputBatch / RnnOption                 run.rs:1128-1132
    State.init/load/back/read/write                      run.rs:477, 1099-1106
    softmax(context, [TensorCpu])                        run.rs:1179
    Tokenizer.encode/decode/token_index_to_bytes         lib.rs:375, run.rs:157-168,856

There is NO fallback: if the shared library is missing or no gfx950 device is present, construction
raises.  Nothing under `oracle/` is ever imported here.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
import time
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RWKV_HIP_LIB") or os.path.join(_HERE, "librwkv_hip.so")   # override: A/B builds (scripts/build_variant.py)


class RwkvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rwkv error {code}: {msg}")
        self.code = code


class _ModelInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("version", "num_layer", "num_emb", "num_hidden", "num_vocab", "num_head",
                                         "head_size", "reserved")]


class _LoraC(C.Structure):
    _fields_ = [("st_bytes", C.c_void_p), ("st_len", C.c_size_t), ("alpha", C.c_float)]


class _LoadDescC(C.Structure):
    _fields_ = [("adapter", C.c_int32), ("quant_layers", C.c_int32), ("quant_type", C.c_int32),
                ("precision", C.c_int32), ("max_batch", C.c_int32), ("token_chunk_size", C.c_int32),
                ("st_bytes", C.c_void_p), ("st_len", C.c_size_t), ("lora", C.POINTER(_LoraC)), ("n_lora", C.c_size_t)]


class _SlotInC(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_uint32)), ("n_tokens", C.c_size_t), ("option", C.c_int32),
                ("reserved", C.c_int32)]


class _SampleC(C.Structure):
    _fields_ = [("top_p", C.c_float), ("top_k", C.c_int32), ("temperature", C.c_float), ("uniform", C.c_float),
                ("adj_tokens", C.POINTER(C.c_uint32)), ("adj_values", C.POINTER(C.c_float)), ("n_adj", C.c_size_t),
                ("kind", C.c_int32), ("tau", C.c_float), ("allow", C.POINTER(C.c_uint8))]


class _GenParamsC(C.Structure):
    _fields_ = [("first_token", C.c_uint32), ("max_tokens", C.c_int32), ("kind", C.c_int32), ("top_p", C.c_float),
                ("top_k", C.c_int32), ("temperature", C.c_float), ("tau", C.c_float), ("presence_penalty", C.c_float),
                ("frequency_penalty", C.c_float), ("penalty_decay", C.c_float), ("miro_target", C.c_float), ("miro_rate", C.c_float),
                ("penalty_tokens", C.POINTER(C.c_uint32)), ("penalty_values", C.POINTER(C.c_float)), ("n_penalty", C.c_size_t),
                ("bias_tokens", C.POINTER(C.c_uint32)), ("bias_values", C.POINTER(C.c_float)), ("n_bias", C.c_size_t),
                ("stop_tokens", C.POINTER(C.c_uint32)), ("n_stop", C.c_size_t), ("allow", C.POINTER(C.c_uint8)),
                ("seed", C.c_uint64), ("stream", C.c_uint32), ("reserved", C.c_uint32)]


class _GenStopsC(C.Structure):
    _fields_ = [("strs", C.POINTER(C.POINTER(C.c_uint8))), ("lens", C.POINTER(C.c_size_t)), ("n", C.c_size_t),
                ("tail", C.POINTER(C.c_uint8)), ("n_tail", C.c_size_t)]


class _SlotOutC(C.Structure):
    _fields_ = [("logits", C.POINTER(C.c_float)), ("logits_capacity_rows", C.c_size_t), ("n_rows", C.c_size_t),
                ("n_consumed", C.c_size_t)]


# every symbol include/rwkv_abi.h declares: (restype, argtypes)
ABI_SYMBOLS = {
    "rwkv_last_error": (C.c_char_p, []),
    "rwkv_abi_version": (C.c_int32, []),
    "rwkv_device_count": (C.c_int32, []),
    "rwkv_device_name": (C.c_int32, [C.c_int32, C.c_char_p, C.c_size_t]),
    "rwkv_model_info_from_st": (C.c_int32, [C.c_void_p, C.c_size_t, C.POINTER(_ModelInfoC)]),
    "rwkv_engine_create": (C.c_int32, [C.POINTER(_LoadDescC), C.POINTER(C.c_void_p)]),
    "rwkv_engine_destroy": (None, [C.c_void_p]),
    "rwkv_engine_save_prefab": (C.c_int32, [C.c_void_p, C.c_char_p]),
    "rwkv_engine_info": (C.c_int32, [C.c_void_p, C.POINTER(_ModelInfoC)]),
    "rwkv_engine_device": (C.c_int32, [C.c_void_p]),
    "rwkv_engine_max_batch": (C.c_int32, [C.c_void_p]),
    "rwkv_engine_token_chunk_size": (C.c_int32, [C.c_void_p]),
    "rwkv_engine_weight_bytes": (C.c_uint64, [C.c_void_p]),
    "rwkv_infer": (C.c_int32, [C.c_void_p, C.POINTER(_SlotInC), C.POINTER(_SlotOutC)]),
    "rwkv_host_alloc": (C.c_int32, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "rwkv_host_free": (None, [C.c_void_p]),
    "rwkv_infer_sample": (C.c_int32, [C.c_void_p, C.POINTER(_SlotInC), C.POINTER(_SampleC), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)]),
    "rwkv_score_rows": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_size_t]),
    "rwkv_infer_score": (C.c_int32, [C.c_void_p, C.POINTER(_SlotInC), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_float)),
                                     C.POINTER(C.c_size_t)]),
    "rwkv_topn_rows": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_size_t]),
    "rwkv_infer_topn": (C.c_int32, [C.c_void_p, C.POINTER(_SlotInC), C.c_int32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_float)),
                                    C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "rwkv_gen_set_topn": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "rwkv_gen_run_topn": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "rwkv_gen_arm": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(_GenParamsC)]),
    "rwkv_gen_arm_prompt": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(_GenParamsC)]),
    "rwkv_gen_prompt_left": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t)]),
    "rwkv_gen_disarm": (C.c_int32, [C.c_void_p, C.c_int32]),
    "rwkv_gen_run": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32)]),
    "rwkv_gen_set_token_bytes": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t]),
    "rwkv_gen_set_stops": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(_GenStopsC)]),
    "rwkv_gen_stop_tail": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "rwkv_gen_uniform": (C.c_int32, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_float)]),
    "rwkv_gen_watch_open": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "rwkv_gen_watch_close": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "rwkv_gen_watch_head": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rwkv_gen_watch_read": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "rwkv_gen_watch_cancel": (C.c_int32, [C.c_void_p, C.c_int32]),
    "rwkv_gen_set_capture": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32]),
    "rwkv_gen_take_item": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rwkv_gen_item_free": (None, [C.c_void_p]),
    "rwkv_gen_item_state": (C.c_void_p, [C.c_void_p]),
    "rwkv_gen_item_back": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rwkv_gen_item_from_host": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rwkv_gen_arm_item": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(_GenParamsC)]),
    "rwkv_dfa_from_table": (C.c_int32, [C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "rwkv_dfa_compile": (C.c_int32, [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "rwkv_dfa_free": (None, [C.c_void_p]),
    "rwkv_dfa_num_states": (C.c_int32, [C.c_void_p]),
    "rwkv_dfa_start": (C.c_int32, [C.c_void_p]),
    "rwkv_dfa_table": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
    "rwkv_dfa_walk": (C.c_int32, [C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
    "rwkv_dfa_allow": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_uint8),
                                   C.c_size_t]),
    "rwkv_dfa_check_live": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_size_t]),
    "rwkv_gen_set_constraint": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "rwkv_gen_constraint_state": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "rwkv_pda_from_table": (C.c_int32, [C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_void_p)]),
    "rwkv_pda_json": (C.c_int32, [C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "rwkv_pda_free": (None, [C.c_void_p]),
    "rwkv_pda_num_states": (C.c_int32, [C.c_void_p]),
    "rwkv_pda_start": (C.c_int32, [C.c_void_p]),
    "rwkv_pda_max_depth": (C.c_int32, [C.c_void_p]),
    "rwkv_pda_table": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
    "rwkv_pda_walk": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint16), C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32),
                                  C.POINTER(C.c_uint16), C.POINTER(C.c_int32)]),
    "rwkv_pda_allow": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint16), C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t,
                                   C.POINTER(C.c_uint8), C.c_size_t]),
    "rwkv_pda_check_live": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint16), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_size_t]),
    "rwkv_gen_set_pda": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_uint16), C.c_int32, C.c_int32]),
    "rwkv_gen_pda_config": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(C.c_int32)]),
    "rwkv_plan_chunk": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "rwkv_state_len": (C.c_size_t, [C.c_void_p]),
    "rwkv_state_shape": (None, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "rwkv_state_init": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "rwkv_state_load": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rwkv_state_back": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rwkv_state_read": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "rwkv_state_write": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rwkv_dstate_free": (None, [C.c_void_p]),
    "rwkv_state_back_layer": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rwkv_state_back_layer_async": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "rwkv_state_sync": (C.c_int32, [C.c_void_p]),
    "rwkv_read_init_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rwkv_softmax": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t]),
    "rwkv_tokenizer_create": (C.c_int32, [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "rwkv_tokenizer_destroy": (None, [C.c_void_p]),
    "rwkv_tokenizer_encode": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
    "rwkv_tokenizer_decode": (C.c_int64, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.c_size_t]),
    "rwkv_tokenizer_token_bytes": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]),
    "rwkv_tokenizer_vocab_size": (C.c_int64, [C.c_void_p]),
    "rwkv_profile_family_name": (C.c_char_p, [C.c_int32]),
    "rwkv_profile_infer": (C.c_int32, [C.c_void_p, C.POINTER(_SlotInC), C.POINTER(_SlotOutC), C.POINTER(C.c_float),
                                       C.POINTER(C.c_int32)]),
    "rwkv_decode_greedy": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_float)]),
    "rwkv_bench_gemm": (C.c_int32, [C.c_int32] * 8 + [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
}
PROFILE_FAMILIES = 8
SCORE_SKIP = 0xFFFFFFFF          # RWKV_SCORE_SKIP: a row that is not scored (its output is NaN)
TOPN_MAX = 32                    # RWKV_TOPN_MAX: the longest top-n list
TOPN_NONE = 0xFFFFFFFF           # RWKV_TOPN_NONE: a place of a list that holds no entry

_lib = None


def lib() -> C.CDLL:
    """Load librwkv_hip.so (built in-tree by `python -m ai00_server_amd.build`).  Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -m ai00_server_amd.build` "
                                    "(there is no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI_SYMBOLS.items():
            fn = getattr(l, name)          # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def _check(code: int):
    if code != 0:
        raise RwkvError(code, lib().rwkv_last_error().decode(errors="replace"))


def _buf(data) -> tuple[C.c_void_p, int, object]:
    """Zero-copy view of bytes / bytearray / numpy / mmap as (ptr, len, keepalive)."""
    if isinstance(data, np.ndarray):
        arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    else:
        arr = np.frombuffer(data, dtype=np.uint8)
    return C.c_void_p(arr.ctypes.data), arr.size, arr


# ------------------------------------------------------------------------------------------------
class ModelVersion(enum.IntEnum):
    V4 = 4
    V5 = 5
    V6 = 6
    V7 = 7


class Quant(enum.IntEnum):       # `Quant` lib.rs:689-704, all four values (SF4: NF4 storage, Student-t code book)
    NONE = 0
    Int8 = 1
    NF4 = 2
    SF4 = 3


class Precision(enum.IntEnum):   # reload.rs:89-94 (+ the raw mode of ABI 7, include/rwkv_abi.h)
    Fp16 = 0                     # f16 operands, the error-carrying launches hi + lo: within 1e-3 at 32 layers (the default)
    Fp32 = 1                     # hi + lo operands everywhere (fp32-class)
    Fp16Raw = 2                  # f16 operands everywhere: fastest, not tolerance-holding at depth


class RnnOption(enum.IntEnum):   # run.rs:716, 819
    Last = 0
    Full = 1
    NoOutput = 2                 # extension (RWKV_OPTION_NONE): state-only jobs such as `/embeddings`; no logits row is produced


@dataclass
class ModelInfo:
    version: ModelVersion
    num_layer: int
    num_emb: int
    num_hidden: int
    num_vocab: int
    num_head: int
    head_size: int


def _info_from_c(c: _ModelInfoC) -> ModelInfo:
    return ModelInfo(ModelVersion(c.version), c.num_layer, c.num_emb, c.num_hidden, c.num_vocab, c.num_head,
                     c.head_size)


class Loader:
    @staticmethod
    def info(st_bytes) -> ModelInfo:
        """`Loader::info(&SafeTensors)` (lib.rs:587, api/file.rs:113-116). Host only, needs no GPU."""
        p, n, keep = _buf(st_bytes)
        out = _ModelInfoC()
        _check(lib().rwkv_model_info_from_st(p, n, C.byref(out)))
        return _info_from_c(out)


def plan_chunk(n_tokens: list[int], token_chunk_size: int) -> list[int]:
    """Tokens of each slot that one `infer` call consumes (host-only mirror of the engine's chunk policy)."""
    n = len(n_tokens)
    a = (C.c_size_t * n)(*n_tokens)
    out = (C.c_int32 * n)()
    _check(lib().rwkv_plan_chunk(n, token_chunk_size, a, out))
    return list(out)


def gen_uniform(seed: int, stream: int, step: int, n: int | None = None):
    """The uniform draw of (seed, stream, step) that a slot armed with `gen_arm` makes (rwkv_gen_uniform; host only, needs no GPU):
    one float, or with `n` the float32 array of the draws step .. step + n - 1."""
    out = np.empty(1 if n is None else int(n), np.float32)
    _check(lib().rwkv_gen_uniform(int(seed), int(stream), int(step), out.size, out.ctypes.data_as(C.POINTER(C.c_float))))
    return float(out[0]) if n is None else out


class GenFinish(enum.IntEnum):   # RWKV_GEN_*: FinishReason::{Stop, Length} run.rs:905-917
    Running = 0
    Stop = 1
    Length = 2
    Handback = 3                 # the slot's stop-string buffer is full: the caller replays its own matcher and goes on per token
    Cancelled = 4                # RWKV_GEN_CANCELLED: the request was cancelled through a watch (`GenWatch.cancel`)


GEN_MAX_STOP_STR, GEN_STOP_LEN, GEN_STOP_BUF, GEN_TOKEN_LEN = 8, 128, 512, 256      # RWKV_GEN_* limits of the device's stop-string matcher
GEN_WATCH_MAX_STEPS = 65536      # RWKV_GEN_WATCH_MAX_STEPS
GEN_WIDE_TOP_K = 1               # RWKV_GEN_WIDE_TOP_K: bit of rwkv_gen_params.reserved that arms Nucleus / Typical with top_k > 256


DFA_MAX_STATES = 4096            # RWKV_DFA_MAX_STATES, the dead state 0 included


class DfaHalt(enum.IntEnum):     # RWKV_DFA_HALT_*
    Final = 0                    # halt when the new state accepts and no byte leads from it to a live state
    Accept = 1                   # halt the first time the new state accepts


def _token_table_arrays(table):
    """(bytes, lens) of a token table as rwkv_gen_set_token_bytes / rwkv_dfa_allow take it: `table[i]` is bytes, or None for an unknown id"""
    lens = np.array([-1 if b is None else len(b) for b in table], np.int32)
    data = np.frombuffer(b"".join(b for b in table if b is not None) or b"\0", np.uint8)
    return data, lens


class Dfa:
    """A byte-level DFA (rwkv_dfa): the constraint resident generation masks on the device, and the same `Formatter` for the per-token
    path (`allow`).  State 0 is dead.  `Dfa.compile(pattern)` takes the anchored regex dialect of include/rwkv_abi.h, `Dfa.from_table`
    any compiler's table.  Host only, needs no GPU.  It covers REGULAR constraints; it is not the reference's kbnf."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def compile(cls, pattern) -> "Dfa":
        data = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
        h = C.c_void_p()
        _check(lib().rwkv_dfa_compile(data, len(data), C.byref(h)))
        return cls(h)

    @classmethod
    def from_table(cls, trans, accepting, start: int = 1) -> "Dfa":
        t = np.ascontiguousarray(trans, dtype=np.uint16).reshape(-1, 256)
        a = np.ascontiguousarray(accepting, dtype=np.uint8).reshape(-1)
        if a.size != t.shape[0]:
            raise RwkvError(-1, "dfa: one accepting flag per row of the table")
        h = C.c_void_p()
        _check(lib().rwkv_dfa_from_table(t.ctypes.data_as(C.POINTER(C.c_uint16)), a.ctypes.data_as(C.POINTER(C.c_uint8)), t.shape[0], int(start),
                                         C.byref(h)))
        return cls(h)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().rwkv_dfa_free(self._h)
            except Exception:
                pass

    @property
    def num_states(self) -> int:
        return int(lib().rwkv_dfa_num_states(self._h))

    @property
    def start(self) -> int:
        return int(lib().rwkv_dfa_start(self._h))

    def table(self):
        """(trans uint16 [num_states, 256], accepting uint8 [num_states])"""
        n = self.num_states
        t, a = np.empty((n, 256), np.uint16), np.empty(n, np.uint8)
        _check(lib().rwkv_dfa_table(self._h, t.ctypes.data_as(C.POINTER(C.c_uint16)), a.ctypes.data_as(C.POINTER(C.c_uint8))))
        return t, a

    def walk(self, state: int, data: bytes) -> int:
        nxt = C.c_int32(0)
        _check(lib().rwkv_dfa_walk(self._h, int(state), bytes(data), len(data), C.byref(nxt)))
        return int(nxt.value)

    def check_live(self, table, state: int | None = None, halt: "DfaHalt" = DfaHalt.Final):
        """The liveness rule of `gen_set_constraint` on the host (rwkv_dfa_check_live): raises RwkvError(-3) when a state the request can come
        to rest in has no single-byte token of `table` that leads on."""
        data, lens = _token_table_arrays(table)
        _check(lib().rwkv_dfa_check_live(self._h, int(self.start if state is None else state), int(halt), lens.ctypes.data_as(C.POINTER(C.c_int32)) if lens.size else None,
                                         data.ctypes.data_as(C.POINTER(C.c_uint8)), lens.size))

    def allow(self, state: int, table, num_vocab: int) -> np.ndarray:
        """The `num_vocab`-byte mask `infer_sample` takes as `allow` (rwkv_dfa_allow): token v is allowed in `state` iff it is in `table`,
        known, non-empty, and its bytes lead to a live state."""
        data, lens = _token_table_arrays(table)
        out = np.empty(int(num_vocab), np.uint8)
        _check(lib().rwkv_dfa_allow(self._h, int(state), data.ctypes.data_as(C.POINTER(C.c_uint8)), lens.ctypes.data_as(C.POINTER(C.c_int32)) if lens.size else None,
                                    lens.size, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out


PDA_MAX_STATES, PDA_MAX_DEPTH, PDA_TOKEN_SPAN, PDA_POP = 4096, 64, 8, 0xFFFF      # RWKV_PDA_*


class PdaHalt(enum.IntEnum):     # RWKV_PDA_HALT_*
    Final = 0                    # halt when the new configuration accepts (empty stack) and its state is END
    Accept = 1                   # halt the first time the new configuration accepts


class PdaJson(enum.IntFlag):     # RWKV_PDA_JSON_*
    Object = 1                   # the top-level value must be an object or an array
    Compact = 2                  # no whitespace outside strings


def _stack_array(stack):
    s = np.ascontiguousarray(list(stack) if stack is not None else [], dtype=np.uint16).reshape(-1)
    return s, (s.ctypes.data_as(C.POINTER(C.c_uint16)) if s.size else None)


class Pda:
    """A byte automaton with a return-state stack (rwkv_pda): the constraint resident generation masks on the device for NESTED formats,
    JSON above all, and the same `Formatter` for the per-token path (`allow`).  State 0 is dead; a configuration is (state, stack).
    `Pda.json(flags, max_depth)` is RFC 8259, `Pda.from_table` takes any compiler's two planes (`act`: 0 plain, PDA_POP pop, else the
    return state a push pushes).  Host only, needs no GPU.  It is not the reference's kbnf: general grammars keep the per-token path."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def json(cls, flags: int = 0, max_depth: int = PDA_MAX_DEPTH) -> "Pda":
        h = C.c_void_p()
        _check(lib().rwkv_pda_json(int(flags), int(max_depth), C.byref(h)))
        return cls(h)

    @classmethod
    def from_table(cls, next, act, accepting, start: int = 1, max_depth: int = PDA_MAX_DEPTH) -> "Pda":
        n = np.ascontiguousarray(next, dtype=np.uint16).reshape(-1, 256)
        a = np.ascontiguousarray(act, dtype=np.uint16).reshape(-1, 256)
        f = np.ascontiguousarray(accepting, dtype=np.uint8).reshape(-1)
        if f.size != n.shape[0] or a.shape != n.shape:
            raise RwkvError(-1, "pda: two planes of one shape and one accepting flag per row")
        h = C.c_void_p()
        _check(lib().rwkv_pda_from_table(n.ctypes.data_as(C.POINTER(C.c_uint16)), a.ctypes.data_as(C.POINTER(C.c_uint16)),
                                         f.ctypes.data_as(C.POINTER(C.c_uint8)), n.shape[0], int(start), int(max_depth), C.byref(h)))
        return cls(h)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().rwkv_pda_free(self._h)
            except Exception:
                pass

    @property
    def num_states(self) -> int:
        return int(lib().rwkv_pda_num_states(self._h))

    @property
    def start(self) -> int:
        return int(lib().rwkv_pda_start(self._h))

    @property
    def max_depth(self) -> int:
        return int(lib().rwkv_pda_max_depth(self._h))

    def table(self):
        """(next uint16 [num_states, 256], act uint16 [num_states, 256], accepting uint8 [num_states])"""
        n = self.num_states
        t, a, f = np.empty((n, 256), np.uint16), np.empty((n, 256), np.uint16), np.empty(n, np.uint8)
        _check(lib().rwkv_pda_table(self._h, t.ctypes.data_as(C.POINTER(C.c_uint16)), a.ctypes.data_as(C.POINTER(C.c_uint16)),
                                    f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return t, a, f

    def walk(self, data: bytes, state: int | None = None, stack=()):
        """(state, stack) `data` behind the configuration (default: the start state, empty stack); state 0 once the walk died.  Bytes,
        not tokens: the span rule of `allow` does not apply."""
        s, sp = _stack_array(stack)
        out = (C.c_uint16 * PDA_MAX_DEPTH)()
        q, d = C.c_int32(0), C.c_int32(0)
        _check(lib().rwkv_pda_walk(self._h, int(self.start if state is None else state), sp, s.size, bytes(data), len(data), C.byref(q), out, C.byref(d)))
        return int(q.value), [int(x) for x in out[:d.value]]

    def check_live(self, table, state: int | None = None, stack=()):
        """The liveness rule of `gen_set_pda` on the host (rwkv_pda_check_live): raises RwkvError(-3) when a state the request can enter has
        no single-byte token of `table` with a plain transition that leads on."""
        data, lens = _token_table_arrays(table)
        s, sp = _stack_array(stack)
        _check(lib().rwkv_pda_check_live(self._h, int(self.start if state is None else state), sp, s.size,
                                         lens.ctypes.data_as(C.POINTER(C.c_int32)) if lens.size else None, data.ctypes.data_as(C.POINTER(C.c_uint8)), lens.size))

    def allow(self, state: int, stack, table, num_vocab: int) -> np.ndarray:
        """The `num_vocab`-byte mask `infer_sample` takes as `allow` (rwkv_pda_allow): token v is allowed in (state, stack) iff it is in
        `table`, known, non-empty, not id 0, and its bytes lead to a live state without owning more than PDA_TOKEN_SPAN stack entries."""
        data, lens = _token_table_arrays(table)
        s, sp = _stack_array(stack)
        out = np.empty(int(num_vocab), np.uint8)
        _check(lib().rwkv_pda_allow(self._h, int(state), sp, s.size, data.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    lens.ctypes.data_as(C.POINTER(C.c_int32)) if lens.size else None, lens.size, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out


def list_adapters() -> list[str]:
    """`list_adapters` (lib.rs:339-349)."""
    l = lib()
    names = []
    for i in range(l.rwkv_device_count()):
        b = C.create_string_buffer(256)
        _check(l.rwkv_device_name(i, b, 256))
        names.append(b.value.decode())
    return names


@dataclass
class RnnInputBatch:             # RnnInputBatch::new(tokens, option) run.rs:1128
    tokens: list = field(default_factory=list)
    option: RnnOption = RnnOption.Last


class RnnInput:
    """RnnInput::new(batches, token_chunk_size) run.rs:1132.  `infer` consumes tokens from it."""

    def __init__(self, batches: list[RnnInputBatch], token_chunk_size: int | None = None):
        self.batches = batches
        self.token_chunk_size = token_chunk_size

    def num_token(self) -> int:   # run.rs:1136
        return sum(len(b.tokens) for b in self.batches)


class State:
    """`dyn State` (bundle.state(), lib.rs:494)."""

    def __init__(self, rt: "Runtime"):
        self._rt = rt

    @property
    def shape(self) -> tuple[int, int, int, int]:
        s = (C.c_size_t * 4)()
        lib().rwkv_state_shape(self._rt._h, s)
        return tuple(int(v) for v in s)

    def _np_shape(self):
        c, r, l, _ = self.shape                                    # V5 / V6 / V7: [C, 66, L, 1]; V4: [C, 5L, 1, 1] (rows 5l .. 5l+4 belong to layer l)
        return (l, r, c)

    @property
    def layer_rows(self) -> int:
        """WKV rows one layer owns in the slab, between its two shift rows (what `embed` returns): 64, V4: 3 (aa, bb, pp)"""
        return 3 if self._rt.info.version == ModelVersion.V4 else self.shape[1] - 2

    def init(self) -> np.ndarray:                                  # run.rs:477, 950
        a = np.empty(self._np_shape(), np.float32)
        _check(lib().rwkv_state_init(self._rt._h, a.ctypes.data))
        return a

    def load(self, tensor: np.ndarray, batch: int) -> None:        # run.rs:1099
        a = np.ascontiguousarray(tensor, np.float32)
        if a.size != int(np.prod(self._np_shape())):
            raise RwkvError(-1, "state tensor has the wrong size")
        _check(lib().rwkv_state_load(self._rt._h, batch, a.ctypes.data))

    def back(self, batch: int) -> np.ndarray:                      # run.rs:1101
        a = np.empty(self._np_shape(), np.float32)
        _check(lib().rwkv_state_back(self._rt._h, batch, a.ctypes.data))
        return a

    def read(self, batch: int) -> "TensorGpu":                     # run.rs:1106
        h = C.c_void_p()
        _check(lib().rwkv_state_read(self._rt._h, batch, C.byref(h)))
        return TensorGpu(h)

    def write(self, tensor: "TensorGpu", batch: int) -> None:      # run.rs:1104
        _check(lib().rwkv_state_write(self._rt._h, batch, tensor._h))

    def embed(self, layer: int, batch: int) -> np.ndarray:
        """One layer's WKV rows [N, C] of a slot (docs/doc-api/openai.md:376-437 `/embeddings`); V4: its aa / bb / pp rows [3, C]."""
        a = np.empty((self.layer_rows, self.shape[0]), np.float32)
        _check(lib().rwkv_state_back_layer(self._rt._h, batch, layer, a.ctypes.data))
        return a

    def embed_async(self, layer: int, batch: int, dst: np.ndarray):
        """The same read-back, not waited for (rwkv_state_back_layer_async): `dst` is a [N, C] float32 view into pinned memory
        (`PinnedArena`), valid after `sync()`.  The slot may be re-used at once."""
        _check(lib().rwkv_state_back_layer_async(self._rt._h, batch, layer, dst.ctypes.data))

    def sync(self):
        _check(lib().rwkv_state_sync(self._rt._h))


class PinnedArena:
    """A float32 array in pinned host memory (rwkv_host_alloc): the destination of asynchronous read-backs (`State.embed_async`)
    and of direct logits copies.  `close()` (or garbage collection) frees it; views must not outlive it."""

    def __init__(self, shape):
        self.shape = tuple(int(x) for x in shape)
        n = int(np.prod(self.shape))
        self._ptr = C.c_void_p()
        _check(lib().rwkv_host_alloc(max(1, n) * 4, C.byref(self._ptr)))
        self.array = np.ctypeslib.as_array(C.cast(self._ptr, C.POINTER(C.c_float)), shape=(max(1, n),))[:n].reshape(self.shape)

    def close(self):
        if self._ptr:
            self.array = None
            lib().rwkv_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GenWatch:
    """A watch on an engine's resident generation (rwkv_gen_watch_*).  `read`, `head` and `cancel` may be called from any thread while
    another sits in `Runtime.gen_run`; `close` belongs to the thread that runs the engine, between runs.  One reader per GenWatch object:
    the cursor lives here."""

    def __init__(self, rt: "Runtime", handle):
        self._rt, self._h, self.cursor, self.lost = rt, handle, 0, 0

    def _handle(self):
        if not self._h:
            raise RwkvError(-1, "the watch is closed")
        return self._h

    def head(self) -> int:
        """records published since the watch was opened"""
        seq = C.c_uint64()
        _check(lib().rwkv_gen_watch_head(self._handle(), C.byref(seq)))
        return int(seq.value)

    def read(self, max_steps: int):
        """The records behind this watch's cursor, at most `max_steps`: (tokens uint32 [n, max_batch], probs float32 [n, max_batch],
        finish int32 [n, max_batch], lost) — the rows of `gen_run`'s outputs as the steps end, 0xFFFFFFFF / NaN where a slot emitted
        nothing; `lost` counts the records a reader that fell behind the ring has skipped in this call (`self.lost` adds them up).
        Never blocks; n may be 0."""
        B, n = self._rt.max_batch, max(int(max_steps), 0)
        toks, probs, fin = np.empty((n, B), np.uint32), np.empty((n, B), np.float32), np.empty((n, B), np.int32)
        cur, got, lost = C.c_uint64(self.cursor), C.c_int32(), C.c_uint64()
        _check(lib().rwkv_gen_watch_read(self._handle(), C.byref(cur), n, toks.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         probs.ctypes.data_as(C.POINTER(C.c_float)), fin.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(got),
                                         C.byref(lost)))
        self.cursor = int(cur.value)
        self.lost += int(lost.value)
        k = int(got.value)
        return toks[:k], probs[:k], fin[:k], int(lost.value)

    def cancel(self, slot: int):
        """The slot's request is gone (rwkv_gen_watch_cancel): a decoding slot ends in the first step that sees the flag, with the token it
        drew there as its last and `GenFinish.Cancelled`; a slot inside its prompt is dropped when the next step is planned."""
        _check(lib().rwkv_gen_watch_cancel(self._handle(), int(slot)))

    def close(self):
        if self._h:
            h, self._h = self._h, None
            self._rt._watch = None
            _check(lib().rwkv_gen_watch_close(self._rt._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TensorGpu:
    """Device-resident state snapshot (`state.read` result); reusable for many `state.write`s.  With `owner` it is a view into memory
    the owner frees (`GenItem.state()`), kept alive by the reference."""

    def __init__(self, h, owner=None):
        self._h = h
        self._owner = owner

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_owner", None) is None:
            try:
                lib().rwkv_dstate_free(self._h)
            except Exception:
                pass
            self._h = None


class GenCapture(enum.IntFlag):   # RWKV_GEN_CAPTURE_*: the two points at which `process` fills the prefix cache
    Prompt = 1                    # run.rs:834-845: the state behind the whole prompt and the prompt's last row
    Finish = 2                    # run.rs:995-1001: the state the STATE RULE prescribes and the row the last token was drawn from


class GenItem:
    """A cached (state, raw logits row) pair on the device (rwkv_gen_item; CachedItem, run.rs:201-223): what `Runtime.gen_take_item`
    hands out and `Runtime.gen_arm_item` starts a slot from.  Immutable; it outlives the slot and the engine that made it, and any
    engine of the same device, model version and dimensions reads it.  `close()` (or garbage collection) frees it."""

    def __init__(self, rt: "Runtime", h):
        self._rt, self._h = rt, h

    def _handle(self):
        if not self._h:
            raise RwkvError(-1, "the item is closed")
        return self._h

    def state(self) -> "TensorGpu":
        """the item's state as `State.write` takes it (rwkv_gen_item_state; a PARTIAL prefix hit); a view, valid while the item is"""
        return TensorGpu(C.c_void_p(lib().rwkv_gen_item_state(self._handle())), owner=self)

    def back(self, rt: "Runtime | None" = None):
        """(state in the layout of `State.back`, row float32 [num_vocab]) on the host (rwkv_gen_item_back), bit for bit"""
        rt = rt or self._rt
        st, row = np.empty(rt.state._np_shape(), np.float32), np.empty(rt.info.num_vocab, np.float32)
        _check(lib().rwkv_gen_item_back(rt._h, self._handle(), st.ctypes.data, row.ctypes.data))
        return st, row

    def row(self) -> np.ndarray:
        """the RAW head row: before penalties, bias, temperature and masks"""
        row = np.empty(self._rt.info.num_vocab, np.float32)
        _check(lib().rwkv_gen_item_back(self._rt._h, self._handle(), None, row.ctypes.data))
        return row

    @staticmethod
    def from_host(rt: "Runtime", state: np.ndarray, row: np.ndarray) -> "GenItem":
        """An item of `rt`'s device from what `back()` returned (rwkv_gen_item_from_host): the way into another engine, or back from disk"""
        st, r = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(row, np.float32).reshape(-1)
        if st.size != int(np.prod(rt.state._np_shape())) or r.size != rt.info.num_vocab:
            raise RwkvError(-1, "state or row has the wrong size")
        h = C.c_void_p()
        _check(lib().rwkv_gen_item_from_host(rt._h, st.ctypes.data, r.ctypes.data, C.byref(h)))
        return GenItem(rt, h)

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            lib().rwkv_gen_item_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelBuilder:
    """`ModelBuilder::new(ctx, st).quant(map).lora(l).build_vN()` + `vN::Bundle::new(model, max_batch)` +
    `TokioRuntime::new(bundle)` (lib.rs:484-516) in one step."""

    def __init__(self, st_bytes, adapter: int = -1):
        self._st = st_bytes
        self._adapter = adapter
        self._quant_layers = 0
        self._quant_type = Quant.NONE
        self._lora: list[tuple[object, float]] = []

    def quant(self, layers: int, quant_type: Quant) -> "ModelBuilder":   # lib.rs:465: (0..quant) -> quant_type
        self._quant_layers, self._quant_type = int(layers), Quant(quant_type)
        return self

    def lora(self, st_bytes, alpha: float) -> "ModelBuilder":           # lib.rs:466-482
        self._lora.append((st_bytes, float(alpha)))
        return self

    def build(self, max_batch: int = 8, token_chunk_size: int = 128,
              precision: Precision = Precision.Fp16) -> "Runtime":
        return Runtime(self, max_batch, token_chunk_size, precision)


class Runtime:
    """`dyn Runtime<Rnn>` (lib.rs:112, 398)."""

    def __init__(self, b: ModelBuilder, max_batch: int, token_chunk_size: int, precision: Precision):
        l = lib()
        p, n, keep = _buf(b._st)
        loras = (_LoraC * max(1, len(b._lora)))()
        keeps = [keep]
        for i, (data, alpha) in enumerate(b._lora):
            lp, ln, lk = _buf(data)
            loras[i] = _LoraC(lp, ln, alpha)
            keeps.append(lk)
        d = _LoadDescC(b._adapter, b._quant_layers, int(b._quant_type), int(precision), max_batch, token_chunk_size,
                       p, n, loras if b._lora else None, len(b._lora))
        h = C.c_void_p()
        _check(l.rwkv_engine_create(C.byref(d), C.byref(h)))
        self._h = h
        self.max_batch = int(l.rwkv_engine_max_batch(h))
        self.token_chunk_size = int(l.rwkv_engine_token_chunk_size(h))    # what the engine was really built with
        ic = _ModelInfoC()
        _check(l.rwkv_engine_info(h, C.byref(ic)))
        self.info = _info_from_c(ic)
        self.state = State(self)
        V = self.info.num_vocab
        self._ins = (_SlotInC * max_batch)()
        self._outs = (_SlotOutC * max_batch)()
        # logits land in ONE pinned block (rwkv_host_alloc): the slots of a call get consecutive pieces of it in slot order, which
        # the engine copies device-to-host in one go; calls that need more rows than the block holds fall back to numpy buffers
        self._arena_rows = token_chunk_size + max_batch
        ap = C.c_void_p()
        _check(l.rwkv_host_alloc(self._arena_rows * V * 4, C.byref(ap)))
        self._arena_ptr = ap
        self._arena = np.ctypeslib.as_array(C.cast(ap, C.POINTER(C.c_float)), shape=(self._arena_rows, V))
        self._views = [None] * max_batch

    def close(self):
        if self._h:
            w = getattr(self, "_watch", None)
            if w is not None:
                w._h = None                                           # the engine's destructor closes an open watch
                self._watch = None
            lib().rwkv_engine_destroy(self._h)
            self._h = None
            self._arena = None
            self._views = []
            lib().rwkv_host_free(self._arena_ptr)
            self._arena_ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device(self) -> int:
        return lib().rwkv_engine_device(self._h)

    @property
    def weight_bytes(self) -> int:
        return int(lib().rwkv_engine_weight_bytes(self._h))

    def save_prefab(self, path: str):
        """`ModelSerialize::serialize(file)` (lib.rs:131-154): the loaded (tiled / quantised / blended) model as one image;
        hand its bytes to `ModelBuilder` like a safetensors file (sniffed by content, lib.rs:585-588)."""
        _check(lib().rwkv_engine_save_prefab(self._h, os.fsencode(path)))

    def _prepare(self, inp: RnnInput):
        if len(inp.batches) != self.max_batch:
            raise RwkvError(-1, f"RnnInput must have max_batch={self.max_batch} entries")
        V = self.info.num_vocab
        keep = []
        needs = [0 if not len(ib.tokens) or ib.option == RnnOption.NoOutput else
                 (1 if ib.option == RnnOption.Last else min(len(ib.tokens), self.token_chunk_size)) for ib in inp.batches]
        pinned = sum(needs) <= self._arena_rows
        row = 0
        for b, ib in enumerate(inp.batches):
            toks = np.asarray(ib.tokens, dtype=np.uint32)
            keep.append(toks)
            if pinned:
                view = self._arena[row:row + needs[b]]
                row += needs[b]
            else:
                view = np.empty((max(1, needs[b]), V), np.float32)
            self._views[b] = view
            self._ins[b] = _SlotInC(toks.ctypes.data_as(C.POINTER(C.c_uint32)) if toks.size else None, toks.size,
                                    int(ib.option), 0)
            self._outs[b] = _SlotOutC(view.ctypes.data_as(C.POINTER(C.c_float)) if needs[b] else None, needs[b], 0, 0)
        return keep

    def _collect(self, inp: RnnInput):
        outs = []
        for b, ib in enumerate(inp.batches):
            o = self._outs[b]
            outs.append(self._views[b][:o.n_rows].copy())         # RnnOutputBatch: [n_rows, V]; empty if n_rows == 0
            # tokens handed over as a numpy array stay one (a view of the rest: the batch jobs keep their documents as arrays, so a step costs
            # no per-token Python work); lists stay lists
            ib.tokens = ib.tokens[o.n_consumed:] if isinstance(ib.tokens, np.ndarray) else list(ib.tokens[o.n_consumed:])
        return inp, outs

    def infer(self, inp: RnnInput):
        """`runtime.infer(input) -> (input, output)` (run.rs:1143): one step over <= token_chunk_size tokens."""
        keep = self._prepare(inp)
        _check(lib().rwkv_infer(self._h, self._ins, self._outs))
        del keep
        return self._collect(inp)

    def infer_sample(self, inp: RnnInput, samplers: list, uniforms: list):
        """On-device sampling front-end (rwkv_infer_sample).  `samplers[b]` is None or an object with `.top_k`,
        `.temperature`, `.adjustments() -> {token: delta_logit}` (penalties and bias merged) and either `.top_p` (nucleus) or
        `.kind = 1` + `.tau` (typical);
        `uniforms[b]` is the draw `fastrand::f32()` would make.  Returns (inp, [(token, prob) or None per slot])."""
        if len(inp.batches) != self.max_batch:
            raise RwkvError(-1, f"RnnInput must have max_batch={self.max_batch} entries")
        B = self.max_batch
        ins, sps = (_SlotInC * B)(), (_SampleC * B)()
        keep = []
        for b, ib in enumerate(inp.batches):
            toks = np.asarray(ib.tokens, dtype=np.uint32)
            keep.append(toks)
            ins[b] = _SlotInC(toks.ctypes.data_as(C.POINTER(C.c_uint32)) if toks.size else None, toks.size, 0, 0)
            s = samplers[b]
            if s is None:
                sps[b] = _SampleC(0.0, 1, 1.0, 0.0, None, None, 0, 0, 0.0, None)
                continue
            adj = s.adjustments()
            at = np.fromiter(adj.keys(), dtype=np.uint32, count=len(adj))
            av = np.fromiter(adj.values(), dtype=np.float32, count=len(adj))
            keep += [at, av]
            kind = int(getattr(s, "kind", 0))                       # 0 nucleus (top_p), 1 typical (tau)
            allow = getattr(s, "allow", None)                       # formatter mask: uint8 [num_vocab], 0 = forbidden (bnf.rs:35-38)
            if allow is not None:
                allow = np.ascontiguousarray(allow, dtype=np.uint8)
                if allow.size != self.info.num_vocab:
                    raise RwkvError(-1, "formatter mask must have num_vocab entries")
                keep.append(allow)
            sps[b] = _SampleC(getattr(s, "top_p", 0.0), s.top_k, s.temperature, uniforms[b],
                              at.ctypes.data_as(C.POINTER(C.c_uint32)) if at.size else None,
                              av.ctypes.data_as(C.POINTER(C.c_float)) if av.size else None, at.size,
                              kind, float(getattr(s, "tau", 0.0)),
                              allow.ctypes.data_as(C.POINTER(C.c_uint8)) if allow is not None else None)
        toks_o, probs_o = (C.c_uint32 * B)(), (C.c_float * B)()
        emitted, consumed = (C.c_uint8 * B)(), (C.c_size_t * B)()
        _check(lib().rwkv_infer_sample(self._h, ins, sps, toks_o, probs_o, emitted, consumed))
        del keep
        out = []
        for b, ib in enumerate(inp.batches):
            ib.tokens = list(ib.tokens[consumed[b]:])
            out.append((int(toks_o[b]), float(probs_o[b])) if emitted[b] else None)
        return inp, out

    def infer_score(self, inp: RnnInput, targets: list):
        """Like `infer`, for slots that are scored instead of read (rwkv_infer_score).  `targets[b]` is None (the slot has no tokens, or
        rides state-only with `RnnOption.NoOutput`) or one target per pending token of slot b: `targets[b][i]` (a token id, or `SCORE_SKIP`) is
        scored on the row that consuming `tokens[b][i]` produces.  Returns (inp, targets, scores): tokens and targets drained by what the call
        consumed, `scores[b]` the float32 ln-probabilities of the rows it consumed (NaN where skipped; empty for a slot that is not scored)."""
        B = self.max_batch
        if len(inp.batches) != B or len(targets) != B:
            raise RwkvError(-1, f"infer_score needs max_batch={B} entries")
        ins = (_SlotInC * B)()
        tp, op = (C.POINTER(C.c_uint32) * B)(), (C.POINTER(C.c_float) * B)()
        keep, scores = [], []
        for b, ib in enumerate(inp.batches):
            toks = np.ascontiguousarray(ib.tokens, dtype=np.uint32).reshape(-1)
            keep.append(toks)
            ins[b] = _SlotInC(toks.ctypes.data_as(C.POINTER(C.c_uint32)) if toks.size else None, toks.size, int(ib.option), 0)
            out = np.empty(0, np.float32)
            if targets[b] is not None:
                tg = np.ascontiguousarray(targets[b], dtype=np.uint32).reshape(-1)
                if tg.size != toks.size:
                    raise RwkvError(-1, f"slot {b}: {tg.size} targets for {toks.size} tokens")
                out = np.full(min(toks.size, self.token_chunk_size), np.nan, np.float32)
                keep.append(tg)
                if tg.size:
                    tp[b] = tg.ctypes.data_as(C.POINTER(C.c_uint32))
                    op[b] = out.ctypes.data_as(C.POINTER(C.c_float))
            scores.append(out)
        consumed = (C.c_size_t * B)()
        _check(lib().rwkv_infer_score(self._h, ins, tp, op, consumed))
        del keep
        rest = []
        for b, ib in enumerate(inp.batches):
            n = int(consumed[b])
            ib.tokens = ib.tokens[n:] if isinstance(ib.tokens, np.ndarray) else list(ib.tokens[n:])
            rest.append(None if targets[b] is None else targets[b][n:])
            scores[b] = scores[b][:n] if targets[b] is not None else scores[b]
        return inp, rest, scores

    def score_rows(self, rows, targets) -> np.ndarray:
        """ln softmax(rows[i])[targets[i]] on the device (rwkv_score_rows; the softmax task's stream and thread): `rows` are host rows of
        num_vocab floats, `targets` token ids or `SCORE_SKIP` (-> NaN).  One float32 per row comes back."""
        ins = [np.ascontiguousarray(r, np.float32).reshape(-1) for r in rows]
        tg = np.ascontiguousarray(targets, dtype=np.uint32).reshape(-1)
        if tg.size != len(ins) or any(r.size != self.info.num_vocab for r in ins):
            raise RwkvError(-1, "score_rows: one target per row, num_vocab values per row")
        out = np.full(len(ins), np.nan, np.float32)
        if not ins:
            return out
        pi = (C.c_void_p * len(ins))(*[r.ctypes.data for r in ins])
        _check(lib().rwkv_score_rows(self._h, pi, tg.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_float)), len(ins)))
        return out

    def topn_rows(self, rows, n: int):
        """The `n` most likely tokens of every row and their ln-probabilities on the device (rwkv_topn_rows; the softmax task's stream and
        thread): `rows` are host rows of num_vocab floats.  Returns (ids uint32 [rows, n], logp float32 [rows, n]): logits descending, ties
        to the lower id, `TOPN_NONE` / -inf where a row has fewer than n entries above -inf, `TOPN_NONE` / NaN on a row holding +inf or NaN;
        every logp is `score_rows`' value for that row and id, bit for bit."""
        ins = [np.ascontiguousarray(r, np.float32).reshape(-1) for r in rows]
        if any(r.size != self.info.num_vocab for r in ins):
            raise RwkvError(-1, "topn_rows: num_vocab values per row")
        w = max(int(n), 0)
        ids, lp = np.full((len(ins), w), TOPN_NONE, np.uint32), np.full((len(ins), w), np.nan, np.float32)
        pi = (C.c_void_p * len(ins))(*[r.ctypes.data for r in ins])
        _check(lib().rwkv_topn_rows(self._h, pi, int(n), ids.ctypes.data_as(C.POINTER(C.c_uint32)), lp.ctypes.data_as(C.POINTER(C.c_float)), len(ins)))
        return ids, lp

    def infer_topn(self, inp: RnnInput, n: int, targets=None, listing=None):
        """`infer` with top-n lists instead of rows (rwkv_infer_topn).  Every slot that has tokens and an option other than
        `RnnOption.NoOutput` lists (`listing[b]` False leaves a slot out: it must then be state-only); a slot keeps its option — `Last`: one
        list when the call exhausts its tokens, `Full`: one per consumed token.  `targets` is None or per slot None / one target per pending
        token of a `Full` slot (a token id or `SCORE_SKIP`): the realised token is scored on its row as `infer_score` does.
        Returns (inp, targets, lists): tokens and targets drained by what the call consumed; `lists[b]` is None for a slot that did not
        list, else (ids uint32 [rows, n], logp float32 [rows, n], tok_logp float32 [rows] or None)."""
        B = self.max_batch
        if len(inp.batches) != B or (targets is not None and len(targets) != B) or (listing is not None and len(listing) != B):
            raise RwkvError(-1, f"infer_topn needs max_batch={B} entries")
        ins = (_SlotInC * B)()
        ip, lp = (C.POINTER(C.c_uint32) * B)(), (C.POINTER(C.c_float) * B)()
        tp, op = (C.POINTER(C.c_uint32) * B)(), (C.POINTER(C.c_float) * B)()
        keep, outs = [], []
        w = max(int(n), 0)
        for b, ib in enumerate(inp.batches):
            toks = np.ascontiguousarray(ib.tokens, dtype=np.uint32).reshape(-1)
            keep.append(toks)
            ins[b] = _SlotInC(toks.ctypes.data_as(C.POINTER(C.c_uint32)) if toks.size else None, toks.size, int(ib.option), 0)
            lists = toks.size and int(ib.option) != int(RnnOption.NoOutput) if listing is None else bool(listing[b])
            if not lists:
                outs.append(None)
                continue
            rows = min(toks.size, self.token_chunk_size) if int(ib.option) == int(RnnOption.Full) else 1
            o = [np.full((rows, w), TOPN_NONE, np.uint32), np.full((rows, w), np.nan, np.float32), None]
            ip[b], lp[b] = o[0].ctypes.data_as(C.POINTER(C.c_uint32)), o[1].ctypes.data_as(C.POINTER(C.c_float))
            if targets is not None and targets[b] is not None:
                tg = np.ascontiguousarray(targets[b], dtype=np.uint32).reshape(-1)
                if tg.size != toks.size:
                    raise RwkvError(-1, f"slot {b}: {tg.size} targets for {toks.size} tokens")
                o[2] = np.full(rows, np.nan, np.float32)
                keep.append(tg)
                tp[b] = tg.ctypes.data_as(C.POINTER(C.c_uint32)) if tg.size else None
                op[b] = o[2].ctypes.data_as(C.POINTER(C.c_float))
            outs.append(o)
        n_rows, consumed = (C.c_size_t * B)(), (C.c_size_t * B)()
        _check(lib().rwkv_infer_topn(self._h, ins, int(n), ip, lp, tp if targets is not None else None, op if targets is not None else None, n_rows, consumed))
        del keep
        rest = None if targets is None else []
        for b, ib in enumerate(inp.batches):
            k, r = int(consumed[b]), int(n_rows[b])
            ib.tokens = ib.tokens[k:] if isinstance(ib.tokens, np.ndarray) else list(ib.tokens[k:])
            if rest is not None:
                rest.append(None if targets[b] is None else targets[b][k:])
            if outs[b] is not None:
                outs[b] = (outs[b][0][:r], outs[b][1][:r], None if outs[b][2] is None else outs[b][2][:r])
        return inp, rest, outs

    # ---- device-resident sampled generation (rwkv_gen_arm / _run / _disarm): the sampler state lives on the device
    def _gen_params(self, slot, first_token, max_tokens, sampler, seed, stream, stop_tokens, bias, allow, wide_top_k=False):
        """rwkv_gen_params from the settings AND the current state of a host-side sampler; returns (struct, arrays to keep alive)"""
        kind = int(getattr(sampler, "kind", 0))
        pen = {} if kind == 2 else dict(getattr(sampler, "penalties", {}))
        bias = dict(bias if bias is not None else getattr(sampler, "bias", {}) or {})
        pt = np.fromiter(pen.keys(), dtype=np.uint32, count=len(pen))
        pv = np.fromiter(pen.values(), dtype=np.float32, count=len(pen))
        bt = np.fromiter(bias.keys(), dtype=np.uint32, count=len(bias))
        bv = np.fromiter(bias.values(), dtype=np.float32, count=len(bias))
        st = np.asarray(list(stop_tokens), dtype=np.uint32)
        u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        if allow is not None:
            allow = np.ascontiguousarray(allow, dtype=np.uint8)
        p = _GenParamsC(int(first_token), int(max_tokens), kind, float(getattr(sampler, "top_p", 0.0)), int(sampler.top_k),
                        float(sampler.temperature), float(getattr(sampler, "tau", 0.0)),
                        float(getattr(sampler, "ap", 0.0)), float(getattr(sampler, "af", 0.0)), float(getattr(sampler, "ad", 1.0)),
                        float(getattr(sampler, "target", 0.0)), float(getattr(sampler, "rate", 0.0)),
                        pt.ctypes.data_as(u32p) if pt.size else None, pv.ctypes.data_as(f32p) if pv.size else None, pt.size,
                        bt.ctypes.data_as(u32p) if bt.size else None, bv.ctypes.data_as(f32p) if bv.size else None, bt.size,
                        st.ctypes.data_as(u32p) if st.size else None, st.size,
                        allow.ctypes.data_as(C.POINTER(C.c_uint8)) if allow is not None else None,
                        int(seed), int(slot if stream is None else stream), GEN_WIDE_TOP_K if wide_top_k else 0)
        return p, (pt, pv, bt, bv, st, allow)

    def gen_arm(self, slot: int, first_token: int, max_tokens: int, sampler, seed: int = 0, stream: int | None = None,
                stop_tokens=(), bias: dict | None = None, allow=None, wide_top_k: bool = False):
        """Arm `slot` with the settings AND the current state of a host-side sampler (`harness.NucleusSampler` / `TypicalSampler` /
        `MirostatSampler`, after its `init(prompt)`): the penalty map it holds is handed over, `sampler.bias` (or `bias`) rides along.
        `first_token` is the token the first step consumes; draw `i` of the slot is `gen_uniform(seed, stream, i)` (stream defaults
        to the slot index).  `allow` exists to be refused: a host-computed formatter mask needs the host between tokens (use `infer_sample`, or a `Dfa` with
        `gen_set_constraint`).
        `wide_top_k` sets RWKV_GEN_WIDE_TOP_K: Nucleus / Typical with `top_k > 256` is armed instead of refused."""
        p, keep = self._gen_params(slot, first_token, max_tokens, sampler, seed, stream, stop_tokens, bias, allow, wide_top_k)
        _check(lib().rwkv_gen_arm(self._h, int(slot), C.byref(p)))
        del keep

    def gen_arm_prompt(self, slot: int, tokens, max_tokens: int, sampler, seed: int = 0, stream: int | None = None,
                       stop_tokens=(), bias: dict | None = None, allow=None, wide_top_k: bool = False):
        """Admission (rwkv_gen_arm_prompt): arm `slot` with the not-yet-consumed tail of its PROMPT instead of a first token.  The
        following `gen_run` steps prefill it next to the decode rows of the slots that are running and draw its first token on the
        device (draw 0 of (seed, stream)) from the prompt's last row.  `sampler` is the host sampler right after `init(prompt)`,
        before any `update`: its penalty map is handed over as in `gen_arm`."""
        p, keep = self._gen_params(slot, 0, max_tokens, sampler, seed, stream, stop_tokens, bias, allow, wide_top_k)
        toks = np.ascontiguousarray(list(tokens), dtype=np.uint32).reshape(-1)
        _check(lib().rwkv_gen_arm_prompt(self._h, int(slot), toks.ctypes.data_as(C.POINTER(C.c_uint32)) if toks.size else None, toks.size,
                                         C.byref(p)))
        del keep

    def gen_arm_item(self, slot: int, item: "GenItem", max_tokens: int, sampler, seed: int = 0, stream: int | None = None,
                     stop_tokens=(), bias: dict | None = None, allow=None, wide_top_k: bool = False):
        """`gen_arm_prompt` for a prompt that is wholly cached (rwkv_gen_arm_item; run.rs:809-810): the slot's state becomes the item's and
        its first token is drawn on the device from the item's row, draw 0 of (seed, stream), in its first step, which consumes nothing.
        `sampler` is the host sampler right after `init(prompt)`, as for `gen_arm_prompt`.  The item is only read."""
        p, keep = self._gen_params(slot, 0, max_tokens, sampler, seed, stream, stop_tokens, bias, allow, wide_top_k)
        _check(lib().rwkv_gen_arm_item(self._h, int(slot), item._handle() if item is not None else None, C.byref(p)))
        del keep

    def gen_set_capture(self, slot: int, what: "GenCapture"):
        """What an armed, unfinished slot keeps for the prefix cache (rwkv_gen_set_capture), set between runs: `GenCapture.Prompt` (only
        while the slot still has prompt left), `GenCapture.Finish`, both, or `GenCapture(0)` to clear.  Re-arming the slot resets it."""
        _check(lib().rwkv_gen_set_capture(self._h, int(slot), int(what)))

    def gen_take_item(self, slot: int, which: "GenCapture") -> "GenItem":
        """The slot's captured item (rwkv_gen_take_item), exactly one flag: `Prompt` once the run that exhausted the prompt has returned,
        `Finish` once the slot has finished.  Each can be taken once; the item is the caller's."""
        h = C.c_void_p()
        _check(lib().rwkv_gen_take_item(self._h, int(slot), int(which), C.byref(h)))
        return GenItem(self, h)

    def gen_prompt_left(self, slot: int) -> int:
        """Prompt tokens of `slot` the resident steps have not consumed yet (0 once it is decoding, or when it is not armed)."""
        left = C.c_size_t(0)
        _check(lib().rwkv_gen_prompt_left(self._h, int(slot), C.byref(left)))
        return int(left.value)

    def gen_disarm(self, slot: int):
        _check(lib().rwkv_gen_disarm(self._h, int(slot)))

    def gen_set_token_bytes(self, table):
        """What `tokenizer.decode([token])` yields per id (rwkv_gen_set_token_bytes; run.rs:856): `table[i]` is the bytes of id i, or None
        for an id that is not in the vocabulary (the decode error of run.rs:858-862: empty word, stop).  `Tokenizer.token_index_to_bytes()`
        with its empty entries turned into None is such a table.  The device matches stop strings over these bytes."""
        data, lens = _token_table_arrays(table)
        _check(lib().rwkv_gen_set_token_bytes(self._h, data.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              lens.ctypes.data_as(C.POINTER(C.c_int32)) if lens.size else None, lens.size))

    def gen_set_stops(self, slot: int, stops, tail: bytes = b""):
        """`GenerateRequest::stop` of an armed, unfinished slot (rwkv_gen_set_stops; run.rs:899-932): matched on the device, inside the
        step, by the reference's own walk.  `tail` is the buffer the caller's matcher (`harness.StopMatcher.tail()`) holds after the tokens
        it handled itself.  Replaces strings and buffer; an empty list clears them."""
        stops = [bytes(s) for s in stops]
        keep = [np.frombuffer(s or b"\0", np.uint8) for s in stops]
        strs = (C.POINTER(C.c_uint8) * max(1, len(stops)))(*[k.ctypes.data_as(C.POINTER(C.c_uint8)) for k in keep])
        lens = (C.c_size_t * max(1, len(stops)))(*[len(s) for s in stops])
        t = np.frombuffer(bytes(tail) or b"\0", np.uint8)
        s = _GenStopsC(strs, lens, len(stops), t.ctypes.data_as(C.POINTER(C.c_uint8)), len(tail))
        _check(lib().rwkv_gen_set_stops(self._h, int(slot), C.byref(s)))
        del keep

    def gen_stop_tail(self, slot: int) -> bytes:
        """The slot's matcher buffer as it stands (rwkv_gen_stop_tail): what a caller that resumes per token hands its own matcher."""
        out = (C.c_uint8 * GEN_STOP_BUF)()
        n = C.c_size_t(0)
        _check(lib().rwkv_gen_stop_tail(self._h, int(slot), out, GEN_STOP_BUF, C.byref(n)))
        return bytes(out[:min(int(n.value), GEN_STOP_BUF)])

    def gen_set_constraint(self, slot: int, dfa: "Dfa | None", state: int | None = None, halt: "DfaHalt" = DfaHalt.Final):
        """The byte-automaton constraint of an armed, unfinished slot (rwkv_gen_set_constraint), set between runs: from then on the slot's
        row is masked, its state advanced and the halt tested on the device.  `state` defaults to the start state (right after
        `gen_arm_prompt`); after `gen_arm` it is the state behind `first_token`.  `dfa=None` clears the constraint."""
        if dfa is None:
            _check(lib().rwkv_gen_set_constraint(self._h, int(slot), None, 0, 0))
            return
        _check(lib().rwkv_gen_set_constraint(self._h, int(slot), dfa._h, int(dfa.start if state is None else state), int(halt)))

    def gen_constraint_state(self, slot: int) -> int:
        """The automaton state behind every token the slot has emitted (rwkv_gen_constraint_state): what a caller that goes on per token
        hands its `harness.DfaFormatter`."""
        st = C.c_int32(0)
        _check(lib().rwkv_gen_constraint_state(self._h, int(slot), C.byref(st)))
        return int(st.value)

    def gen_set_pda(self, slot: int, pda: "Pda | None", state: int | None = None, stack=(), halt: "PdaHalt" = PdaHalt.Final):
        """The stack-automaton constraint of an armed, unfinished slot (rwkv_gen_set_pda), set between runs: from then on the slot's row is
        masked, the drawn token committed to its configuration and the halt tested on the device.  (`state`, `stack`) defaults to the start
        state with an empty stack (right after `gen_arm_prompt`); after `gen_arm` or a hand-over it is the caller's own.  `pda=None` clears
        it.  A slot holds a `Dfa` or a `Pda`, not both."""
        if pda is None:
            _check(lib().rwkv_gen_set_pda(self._h, int(slot), None, 0, None, 0, 0))
            return
        s, sp = _stack_array(stack)
        _check(lib().rwkv_gen_set_pda(self._h, int(slot), pda._h, int(pda.start if state is None else state), sp, s.size, int(halt)))

    def gen_pda_config(self, slot: int):
        """(state, stack) behind every token the slot has emitted (rwkv_gen_pda_config; (0, []) without a stack constraint): what a caller
        that goes on per token hands its `harness.PdaFormatter`."""
        out = (C.c_uint16 * PDA_MAX_DEPTH)()
        q, d = C.c_int32(0), C.c_int32(0)
        _check(lib().rwkv_gen_pda_config(self._h, int(slot), C.byref(q), out, PDA_MAX_DEPTH, C.byref(d)))
        return int(q.value), [int(x) for x in out[:d.value]]

    def gen_set_topn(self, slot: int, n: int):
        """An armed, unfinished slot lists its `n` (0 .. TOPN_MAX; 0 = off) most likely tokens of the RAW model row — before penalties, bias,
        temperature and any constraint mask — with every token it emits from now on (rwkv_gen_set_topn).  Re-arming the slot resets it."""
        _check(lib().rwkv_gen_set_topn(self._h, int(slot), int(n)))

    def gen_run(self, n_steps: int, top: int = 0):
        """Up to `n_steps` decode steps of every armed, unfinished slot without a host turn-around.  Returns (tokens uint32
        [n_steps, max_batch] with 0xFFFFFFFF where a slot emitted nothing, probs float32 of the same shape with NaN there,
        n_emitted [max_batch] of this call, finish [max_batch] of `GenFinish`).
        With `top` > 0 (rwkv_gen_run_topn; `top` >= every armed slot's `gen_set_topn` n) three more arrays follow: tok_logp float32
        [n_steps, max_batch], the raw ln-probability of the emitted token, and top_ids uint32 / top_logp float32 [n_steps, max_batch, top],
        every slot's list padded with `TOPN_NONE` / -inf up to `top`; `TOPN_NONE` / NaN where a slot emitted nothing."""
        B = self.max_batch
        toks = np.empty((n_steps, B), np.uint32)
        probs = np.empty((n_steps, B), np.float32)
        n_emitted, finish = np.zeros(B, np.int32), np.zeros(B, np.int32)
        i32p, u32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        if not top:
            _check(lib().rwkv_gen_run(self._h, int(n_steps), toks.ctypes.data_as(u32p), probs.ctypes.data_as(f32p),
                                      n_emitted.ctypes.data_as(i32p), finish.ctypes.data_as(i32p)))
            return toks, probs, n_emitted, finish
        w = max(int(top), 0)
        tok_logp = np.full((n_steps, B), np.nan, np.float32)
        top_ids, top_logp = np.full((n_steps, B, w), TOPN_NONE, np.uint32), np.full((n_steps, B, w), np.nan, np.float32)
        _check(lib().rwkv_gen_run_topn(self._h, int(n_steps), toks.ctypes.data_as(u32p), probs.ctypes.data_as(f32p), n_emitted.ctypes.data_as(i32p),
                                       finish.ctypes.data_as(i32p), int(top), tok_logp.ctypes.data_as(f32p), top_ids.ctypes.data_as(u32p),
                                       top_logp.ctypes.data_as(f32p)))
        return toks, probs, n_emitted, finish, tok_logp, top_ids, top_logp

    def gen_watch_open(self, ring_steps: int) -> "GenWatch":
        """Open the engine's watch (rwkv_gen_watch_open; at most one, between runs): from now on every step of `gen_run` publishes a record
        into a ring of `ring_steps` that ANOTHER THREAD reads while the run goes on — ctypes releases the GIL inside `gen_run` — and
        through which it cancels slots."""
        h = C.c_void_p()
        _check(lib().rwkv_gen_watch_open(self._h, int(ring_steps), C.byref(h)))
        self._watch = GenWatch(self, h)
        return self._watch

    gen_uniform = staticmethod(gen_uniform)

    # ---- measurement loops (bench.py): the same ABI calls with every per-step Python object hoisted out, so that the rate is
    # the library's, not the interpreter's
    def serve_loop_logits(self, first_tokens, n_steps: int) -> float:
        """`n_steps` single-token steps of `len(first_tokens)` slots through rwkv_infer with the logits of every slot copied to
        the (pinned) host block each step, as run.rs:809-832 receives them; returns seconds.  The token fed is the slot's first
        token every step: the arg-max over 65 536 floats per slot on the host is the sampler's cost, not the transport's."""
        B = len(first_tokens)
        toks = np.asarray(first_tokens, dtype=np.uint32).copy()
        for b in range(self.max_batch):
            self._ins[b] = _SlotInC(C.cast(toks.ctypes.data + 4 * b, C.POINTER(C.c_uint32)) if b < B else None, 1 if b < B else 0, 0, 0)
            self._outs[b] = _SlotOutC(self._arena[b:b + 1].ctypes.data_as(C.POINTER(C.c_float)) if b < B else None, 1 if b < B else 0, 0, 0)
        l, h, ins, outs = lib(), self._h, self._ins, self._outs
        _check(l.rwkv_infer(h, ins, outs))
        t = time.perf_counter()
        for _ in range(n_steps):
            rc = l.rwkv_infer(h, ins, outs)
            if rc:
                _check(rc)
        return time.perf_counter() - t

    def serve_loop_sample(self, first_tokens, n_steps: int, top_p=0.5, top_k=128, temperature=1.0, seed=0) -> float:
        """The same loop through rwkv_infer_sample (nucleus defaults of the reference, sampler/nucleus.rs:25-35): 8 bytes per slot
        come back instead of 256 KiB, and the token the device picked is fed to the next step.  Returns seconds."""
        B = len(first_tokens)
        toks = np.asarray(first_tokens, dtype=np.uint32).copy()
        u = np.random.default_rng(seed).random((n_steps + 1, self.max_batch))
        ins, sps = (_SlotInC * self.max_batch)(), (_SampleC * self.max_batch)()
        for b in range(self.max_batch):
            ins[b] = _SlotInC(C.cast(toks.ctypes.data + 4 * b, C.POINTER(C.c_uint32)) if b < B else None, 1 if b < B else 0, 0, 0)
            sps[b] = _SampleC(top_p, top_k, temperature, 0.0, None, None, 0, 0, 0.0, None)
        toks_o, probs_o = (C.c_uint32 * self.max_batch)(), (C.c_float * self.max_batch)()
        emitted, consumed = (C.c_uint8 * self.max_batch)(), (C.c_size_t * self.max_batch)()
        out_view = np.ctypeslib.as_array(toks_o)
        l, h = lib(), self._h
        _check(l.rwkv_infer_sample(h, ins, sps, toks_o, probs_o, emitted, consumed))
        t = time.perf_counter()
        sp_view = np.frombuffer(sps, dtype=np.dtype({"names": ["uniform"], "formats": [np.float32],
                                                     "offsets": [_SampleC.uniform.offset], "itemsize": C.sizeof(_SampleC)}))
        u32 = u.astype(np.float32)
        for s_ in range(n_steps):
            sp_view["uniform"][:B] = u32[s_, :B]                 # one strided store instead of B attribute writes
            rc = l.rwkv_infer_sample(h, ins, sps, toks_o, probs_o, emitted, consumed)
            if rc:
                _check(rc)
            toks[:B] = out_view[:B]
        return time.perf_counter() - t

    def profile_infer(self, inp: RnnInput):
        keep = self._prepare(inp)
        ms = (C.c_float * PROFILE_FAMILIES)()
        n = (C.c_int32 * PROFILE_FAMILIES)()
        _check(lib().rwkv_profile_infer(self._h, self._ins, self._outs, ms, n))
        del keep
        inp, outs = self._collect(inp)
        fam = {lib().rwkv_profile_family_name(i).decode(): (float(ms[i]), int(n[i])) for i in range(PROFILE_FAMILIES)
               if lib().rwkv_profile_family_name(i)}
        return inp, outs, fam

    def decode_greedy(self, first_tokens, n_steps: int):
        """Device-resident greedy decode of `len(first_tokens)` slots; returns (tokens [n_steps, n_slots], ms)."""
        ft = np.asarray(first_tokens, dtype=np.uint32)
        out = np.empty((n_steps, ft.size), np.uint32)
        ms = C.c_float()
        _check(lib().rwkv_decode_greedy(self._h, ft.size, ft.ctypes.data_as(C.POINTER(C.c_uint32)), n_steps,
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms)))
        return out, float(ms.value)

    def read_state(self, st_bytes) -> np.ndarray:
        """`vN::read_state(context, info, model)` (lib.rs:378-389)."""
        p, n, keep = _buf(st_bytes)
        a = np.empty(self.state._np_shape(), np.float32)
        _check(lib().rwkv_read_init_state(self._h, p, n, a.ctypes.data))
        return a


def bench_gemm(rows: int, K: int, fmt: int, T: int, hilo: bool = False, spb: int = 0, nmat: int = 16,
               iters: int = 200) -> tuple[float, float]:
    """Kernel microbench hook: (microseconds per launch inside a captured graph, blocks per launch)."""
    us, lds = C.c_float(), C.c_float()
    _check(lib().rwkv_bench_gemm(rows, K, fmt, T, int(hilo), spb, nmat, iters, C.byref(us), C.byref(lds)))
    return float(us.value), float(lds.value)


def softmax(rt: Runtime, tensors: list[np.ndarray]) -> list[np.ndarray]:
    """`web_rwkv::runtime::softmax::softmax(&context, Vec<TensorCpu>)` (run.rs:1179)."""
    if not tensors:
        return []
    ins = [np.ascontiguousarray(t, np.float32).reshape(-1) for t in tensors]
    outs = [np.empty_like(t) for t in ins]
    pi = (C.c_void_p * len(ins))(*[t.ctypes.data for t in ins])
    po = (C.c_void_p * len(ins))(*[t.ctypes.data for t in outs])
    _check(lib().rwkv_softmax(rt._h, pi, po, len(ins)))
    return outs


class Tokenizer:
    """`Tokenizer::new(&contents)` (lib.rs:375)."""

    def __init__(self, vocab_json: str | bytes):
        data = vocab_json.encode() if isinstance(vocab_json, str) else bytes(vocab_json)
        h = C.c_void_p()
        _check(lib().rwkv_tokenizer_create(data, len(data), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().rwkv_tokenizer_destroy(self._h)
            except Exception:
                pass

    def encode(self, text: bytes) -> list[int]:                     # run.rs:157
        n = lib().rwkv_tokenizer_encode(self._h, text, len(text), None, 0)
        if n < 0:
            raise RwkvError(int(n), "no matching token found")
        buf = (C.c_uint32 * max(1, n))()
        lib().rwkv_tokenizer_encode(self._h, text, len(text), buf, n)
        return list(buf[:n])

    def decode(self, tokens) -> bytes:                              # run.rs:856
        t = np.asarray(tokens, dtype=np.uint32)
        p = t.ctypes.data_as(C.POINTER(C.c_uint32))
        n = lib().rwkv_tokenizer_decode(self._h, p, t.size, None, 0)
        if n < 0:
            raise RwkvError(int(n), "token index out of range")
        buf = C.create_string_buffer(max(1, n))
        lib().rwkv_tokenizer_decode(self._h, p, t.size, buf, n)
        return buf.raw[:n]

    def token_index_to_bytes(self) -> list[bytes]:                  # sampler/bnf.rs:15
        out = []
        for i in range(lib().rwkv_tokenizer_vocab_size(self._h)):
            n = lib().rwkv_tokenizer_token_bytes(self._h, i, None, 0)
            if n < 0:
                out.append(b"")
                continue
            buf = C.create_string_buffer(max(1, n))
            lib().rwkv_tokenizer_token_bytes(self._h, i, buf, n)
            out.append(buf.raw[:n])
        return out
