//! Raw bindings of `include/rwkv_abi.h` (ABI version 9), one `pub fn` per export, in the header's order.
//! tests/test_abi_cpu.py diffs this file against the header (names and argument counts) and against the built library.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_float, c_void};

pub const RWKV_ABI_VERSION: i32 = 9;

pub type rwkv_status = i32;
pub const RWKV_V4: i32 = 4;              // rwkv_model_info.version of an RWKV-4 model (5 / 6 / 7 are matched as plain integers)
pub const RWKV_OK: rwkv_status = 0;
pub const RWKV_ERR_INVALID: rwkv_status = -1;
pub const RWKV_ERR_FORMAT: rwkv_status = -2;
pub const RWKV_ERR_UNSUPPORTED: rwkv_status = -3;
pub const RWKV_ERR_DEVICE: rwkv_status = -4;
pub const RWKV_ERR_OOM: rwkv_status = -5;
pub const RWKV_ERR_NO_STATE: rwkv_status = -6;

pub const RWKV_QUANT_NONE: i32 = 0;
pub const RWKV_QUANT_INT8: i32 = 1;
pub const RWKV_QUANT_NF4: i32 = 2;
pub const RWKV_QUANT_SF4: i32 = 3;
pub const RWKV_PRECISION_FP16: i32 = 0;
pub const RWKV_PRECISION_FP32: i32 = 1;
pub const RWKV_PRECISION_FP16_RAW: i32 = 2;
pub const RWKV_ADAPTER_AUTO: i32 = -1;
pub const RWKV_ADAPTER_ECONOMICAL: i32 = -2;
pub const RWKV_OPTION_LAST: i32 = 0;
pub const RWKV_OPTION_FULL: i32 = 1;
pub const RWKV_OPTION_NONE: i32 = 2;
pub const RWKV_SAMPLER_NUCLEUS: i32 = 0;
pub const RWKV_SAMPLER_TYPICAL: i32 = 1;
pub const RWKV_SAMPLER_MIROSTAT: i32 = 2;
pub const RWKV_GEN_MAX_STOP: usize = 8;
pub const RWKV_GEN_RUNNING: i32 = 0;
pub const RWKV_GEN_STOP: i32 = 1;
pub const RWKV_GEN_LENGTH: i32 = 2;
pub const RWKV_GEN_HANDBACK: i32 = 3;
pub const RWKV_GEN_CANCELLED: i32 = 4;
pub const RWKV_GEN_WATCH_MAX_STEPS: i32 = 65536;
pub const RWKV_GEN_MAX_STOP_STR: usize = 8;
pub const RWKV_GEN_STOP_LEN: usize = 128;
pub const RWKV_GEN_STOP_BUF: usize = 512;
pub const RWKV_GEN_TOKEN_LEN: usize = 256;
pub const RWKV_GEN_WIDE_TOP_K: u32 = 1;
pub const RWKV_DFA_MAX_STATES: usize = 4096;
pub const RWKV_DFA_HALT_FINAL: i32 = 0;
pub const RWKV_DFA_HALT_ACCEPT: i32 = 1;
pub const RWKV_PDA_MAX_STATES: usize = 4096;
pub const RWKV_PDA_MAX_DEPTH: usize = 64;
pub const RWKV_PDA_TOKEN_SPAN: usize = 8;
pub const RWKV_PDA_POP: u16 = 65535;
pub const RWKV_PDA_HALT_FINAL: i32 = 0;
pub const RWKV_PDA_HALT_ACCEPT: i32 = 1;
pub const RWKV_PDA_JSON_OBJECT: u32 = 1;
pub const RWKV_PDA_JSON_COMPACT: u32 = 2;
pub const RWKV_PROFILE_FAMILIES: usize = 8;
pub const RWKV_SCORE_SKIP: u32 = 4294967295;
pub const RWKV_TOPN_MAX: i32 = 32;
pub const RWKV_TOPN_NONE: u32 = 4294967295;

#[repr(C)] pub struct rwkv_engine { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_dstate { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_tokenizer { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_dfa { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_pda { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_gen_watch { _p: [u8; 0] }
#[repr(C)] pub struct rwkv_gen_item { _p: [u8; 0] }
pub const RWKV_GEN_CAPTURE_PROMPT: u32 = 1;
pub const RWKV_GEN_CAPTURE_FINISH: u32 = 2;

#[repr(C)] #[derive(Debug, Default, Clone, Copy, PartialEq, Eq)]
pub struct rwkv_model_info { pub version: i32, pub num_layer: i32, pub num_emb: i32, pub num_hidden: i32,
                             pub num_vocab: i32, pub num_head: i32, pub head_size: i32, pub reserved: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_lora_desc { pub st_bytes: *const u8, pub st_len: usize, pub alpha: c_float }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_load_desc { pub adapter: i32, pub quant_layers: i32, pub quant_type: i32, pub precision: i32,
                            pub max_batch: i32, pub token_chunk_size: i32,
                            pub st_bytes: *const u8, pub st_len: usize,
                            pub lora: *const rwkv_lora_desc, pub n_lora: usize }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_slot_input { pub tokens: *const u32, pub n_tokens: usize, pub option: i32, pub reserved: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_slot_output { pub logits: *mut f32, pub logits_capacity_rows: usize, pub n_rows: usize, pub n_consumed: usize }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_sample_params { pub top_p: c_float, pub top_k: i32, pub temperature: c_float, pub uniform: c_float,
                                pub adj_tokens: *const u32, pub adj_values: *const c_float, pub n_adj: usize,
                                pub kind: i32, pub tau: c_float, pub allow: *const u8 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_gen_params { pub first_token: u32, pub max_tokens: i32, pub kind: i32, pub top_p: c_float, pub top_k: i32,
                             pub temperature: c_float, pub tau: c_float, pub presence_penalty: c_float, pub frequency_penalty: c_float,
                             pub penalty_decay: c_float, pub miro_target: c_float, pub miro_rate: c_float,
                             pub penalty_tokens: *const u32, pub penalty_values: *const c_float, pub n_penalty: usize,
                             pub bias_tokens: *const u32, pub bias_values: *const c_float, pub n_bias: usize,
                             pub stop_tokens: *const u32, pub n_stop: usize, pub allow: *const u8,
                             pub seed: u64, pub stream: u32, pub reserved: u32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rwkv_gen_stops { pub strs: *const *const u8, pub lens: *const usize, pub n: usize, pub tail: *const u8, pub n_tail: usize }

extern "C" {
    // errors / version / adapters  (lib.rs:339-349)
    pub fn rwkv_last_error() -> *const c_char;
    pub fn rwkv_abi_version() -> i32;
    pub fn rwkv_device_count() -> i32;
    pub fn rwkv_device_name(index: i32, buf: *mut c_char, buf_len: usize) -> rwkv_status;
    // Loader::info, load / unload / save  (lib.rs:587, 391-516, 652-656, 131-154)
    pub fn rwkv_model_info_from_st(st_bytes: *const u8, st_len: usize, out: *mut rwkv_model_info) -> rwkv_status;
    pub fn rwkv_engine_create(desc: *const rwkv_load_desc, out: *mut *mut rwkv_engine) -> rwkv_status;
    pub fn rwkv_engine_destroy(e: *mut rwkv_engine);
    pub fn rwkv_engine_save_prefab(e: *mut rwkv_engine, path: *const c_char) -> rwkv_status;
    pub fn rwkv_engine_info(e: *const rwkv_engine, out: *mut rwkv_model_info) -> rwkv_status;
    pub fn rwkv_engine_device(e: *const rwkv_engine) -> i32;
    pub fn rwkv_engine_max_batch(e: *const rwkv_engine) -> i32;
    pub fn rwkv_engine_token_chunk_size(e: *const rwkv_engine) -> i32;
    pub fn rwkv_engine_weight_bytes(e: *const rwkv_engine) -> u64;
    // runtime.infer  (run.rs:1128-1156) and the pinned buffers its logits land in
    pub fn rwkv_infer(e: *mut rwkv_engine, inp: *const rwkv_slot_input, out: *mut rwkv_slot_output) -> rwkv_status;
    pub fn rwkv_host_alloc(bytes: usize, out: *mut *mut c_void) -> rwkv_status;
    pub fn rwkv_host_free(p: *mut c_void);
    pub fn rwkv_plan_chunk(max_batch: i32, token_chunk_size: i32, n_tokens: *const usize, consumed: *mut i32) -> rwkv_status;
    // State  (run.rs:477, 950, 987, 1099-1106) and the /embeddings slice
    pub fn rwkv_state_len(e: *const rwkv_engine) -> usize;
    pub fn rwkv_state_shape(e: *const rwkv_engine, shape: *mut usize);
    pub fn rwkv_state_init(e: *const rwkv_engine, dst: *mut f32) -> rwkv_status;
    pub fn rwkv_state_load(e: *mut rwkv_engine, slot: i32, src: *const f32) -> rwkv_status;
    pub fn rwkv_state_back(e: *mut rwkv_engine, slot: i32, dst: *mut f32) -> rwkv_status;
    pub fn rwkv_state_read(e: *mut rwkv_engine, slot: i32, snap: *mut *mut rwkv_dstate) -> rwkv_status;
    pub fn rwkv_state_write(e: *mut rwkv_engine, slot: i32, snap: *const rwkv_dstate) -> rwkv_status;
    pub fn rwkv_dstate_free(snap: *mut rwkv_dstate);
    pub fn rwkv_state_back_layer(e: *mut rwkv_engine, slot: i32, layer: i32, dst: *mut f32) -> rwkv_status;
    pub fn rwkv_state_back_layer_async(e: *mut rwkv_engine, slot: i32, layer: i32, dst: *mut f32) -> rwkv_status;
    pub fn rwkv_state_sync(e: *mut rwkv_engine) -> rwkv_status;
    pub fn rwkv_read_init_state(e: *const rwkv_engine, st_bytes: *const u8, st_len: usize, dst: *mut f32) -> rwkv_status;
    // softmax task  (run.rs:1178-1183)
    pub fn rwkv_softmax(e: *mut rwkv_engine, inp: *const *const f32, out: *const *mut f32, n_rows: usize) -> rwkv_status;
    // scoring on the device: perplexity / Choose (run.rs:699-755, 936-982)
    pub fn rwkv_score_rows(e: *mut rwkv_engine, inp: *const *const f32, targets: *const u32, out_logp: *mut c_float, n_rows: usize) -> rwkv_status;
    pub fn rwkv_infer_score(e: *mut rwkv_engine, inp: *const rwkv_slot_input, targets: *const *const u32, out_logp: *const *mut c_float,
                            n_consumed: *mut usize) -> rwkv_status;
    // top-n lists on the device: the `top_logprobs` of a completion
    pub fn rwkv_topn_rows(e: *mut rwkv_engine, inp: *const *const f32, n: i32, out_ids: *mut u32, out_logp: *mut c_float, n_rows: usize) -> rwkv_status;
    pub fn rwkv_infer_topn(e: *mut rwkv_engine, inp: *const rwkv_slot_input, n: i32, out_ids: *const *mut u32, out_logp: *const *mut c_float,
                           targets: *const *const u32, out_tok_logp: *const *mut c_float, n_rows: *mut usize, n_consumed: *mut usize) -> rwkv_status;
    pub fn rwkv_gen_set_topn(e: *mut rwkv_engine, slot: i32, n: i32) -> rwkv_status;
    pub fn rwkv_gen_run_topn(e: *mut rwkv_engine, n_steps: i32, out_tokens: *mut u32, out_probs: *mut c_float, n_emitted: *mut i32, finish: *mut i32,
                             n_top: i32, out_tok_logp: *mut c_float, out_top_ids: *mut u32, out_top_logp: *mut c_float) -> rwkv_status;
    // on-device sampling front-end (run.rs:664-697 + sampler/*.rs)
    pub fn rwkv_infer_sample(e: *mut rwkv_engine, inp: *const rwkv_slot_input, sp: *const rwkv_sample_params, out_tokens: *mut u32,
                             out_probs: *mut c_float, emitted: *mut u8, n_consumed: *mut usize) -> rwkv_status;
    // device-resident sampled generation: the decode loop of `process` with the samplers on the device (run.rs:788-1020, sampler/*.rs)
    pub fn rwkv_gen_arm(e: *mut rwkv_engine, slot: i32, p: *const rwkv_gen_params) -> rwkv_status;
    pub fn rwkv_gen_arm_prompt(e: *mut rwkv_engine, slot: i32, tokens: *const u32, n_tokens: usize, p: *const rwkv_gen_params) -> rwkv_status;
    pub fn rwkv_gen_prompt_left(e: *const rwkv_engine, slot: i32, left: *mut usize) -> rwkv_status;
    pub fn rwkv_gen_disarm(e: *mut rwkv_engine, slot: i32) -> rwkv_status;
    pub fn rwkv_gen_run(e: *mut rwkv_engine, n_steps: i32, out_tokens: *mut u32, out_probs: *mut c_float, n_emitted: *mut i32,
                        finish: *mut i32) -> rwkv_status;
    // stop strings matched on the device (run.rs:855-869, 899-932, 990-1011)
    pub fn rwkv_gen_set_token_bytes(e: *mut rwkv_engine, bytes: *const u8, lens: *const i32, n_tokens: usize) -> rwkv_status;
    pub fn rwkv_gen_set_stops(e: *mut rwkv_engine, slot: i32, s: *const rwkv_gen_stops) -> rwkv_status;
    pub fn rwkv_gen_stop_tail(e: *mut rwkv_engine, slot: i32, out: *mut u8, cap: usize, len: *mut usize) -> rwkv_status;
    pub fn rwkv_gen_uniform(seed: u64, stream: u32, first_step: u32, n: usize, out: *mut c_float) -> rwkv_status;
    // a watch: open / close on the infer thread between runs; head / read / cancel from any thread, no HIP call behind them
    pub fn rwkv_gen_watch_open(e: *mut rwkv_engine, ring_steps: i32, out: *mut *mut rwkv_gen_watch) -> rwkv_status;
    pub fn rwkv_gen_watch_close(e: *mut rwkv_engine, w: *mut rwkv_gen_watch) -> rwkv_status;
    pub fn rwkv_gen_watch_head(w: *const rwkv_gen_watch, seq: *mut u64) -> rwkv_status;
    pub fn rwkv_gen_watch_read(w: *mut rwkv_gen_watch, cursor: *mut u64, max_steps: i32, tokens: *mut u32, probs: *mut c_float, finish: *mut i32,
                               n_steps: *mut i32, lost: *mut u64) -> rwkv_status;
    pub fn rwkv_gen_watch_cancel(w: *mut rwkv_gen_watch, slot: i32) -> rwkv_status;
    pub fn rwkv_gen_set_capture(e: *mut rwkv_engine, slot: i32, what: u32) -> rwkv_status;
    pub fn rwkv_gen_take_item(e: *mut rwkv_engine, slot: i32, which: u32, out: *mut *mut rwkv_gen_item) -> rwkv_status;
    pub fn rwkv_gen_item_free(it: *mut rwkv_gen_item);
    pub fn rwkv_gen_item_state(it: *const rwkv_gen_item) -> *const rwkv_dstate;
    pub fn rwkv_gen_item_back(e: *mut rwkv_engine, it: *const rwkv_gen_item, state_dst: *mut c_float, row_dst: *mut c_float) -> rwkv_status;
    pub fn rwkv_gen_item_from_host(e: *mut rwkv_engine, state: *const c_float, row: *const c_float, out: *mut *mut rwkv_gen_item) -> rwkv_status;
    pub fn rwkv_gen_arm_item(e: *mut rwkv_engine, slot: i32, it: *const rwkv_gen_item, p: *const rwkv_gen_params) -> rwkv_status;
    // `Formatter` for regular constraints: byte-level DFAs, masked and advanced on the device (sampler/bnf.rs:34-48, run.rs:676-680, 892-897, 990)
    pub fn rwkv_dfa_from_table(trans: *const u16, accepting: *const u8, n_states: i32, start: i32, out: *mut *mut rwkv_dfa) -> rwkv_status;
    pub fn rwkv_dfa_compile(pattern: *const u8, len: usize, out: *mut *mut rwkv_dfa) -> rwkv_status;
    pub fn rwkv_dfa_free(d: *mut rwkv_dfa);
    pub fn rwkv_dfa_num_states(d: *const rwkv_dfa) -> i32;
    pub fn rwkv_dfa_start(d: *const rwkv_dfa) -> i32;
    pub fn rwkv_dfa_table(d: *const rwkv_dfa, trans: *mut u16, accepting: *mut u8) -> rwkv_status;
    pub fn rwkv_dfa_walk(d: *const rwkv_dfa, state: i32, bytes: *const u8, n: usize, next: *mut i32) -> rwkv_status;
    pub fn rwkv_dfa_allow(d: *const rwkv_dfa, state: i32, bytes: *const u8, lens: *const i32, n_tokens: usize, allow: *mut u8,
                          num_vocab: usize) -> rwkv_status;
    pub fn rwkv_dfa_check_live(d: *const rwkv_dfa, state: i32, halt_mode: i32, lens: *const i32, bytes: *const u8, n_tokens: usize) -> rwkv_status;
    pub fn rwkv_gen_set_constraint(e: *mut rwkv_engine, slot: i32, dfa: *const rwkv_dfa, state: i32, halt_mode: i32) -> rwkv_status;
    pub fn rwkv_gen_constraint_state(e: *mut rwkv_engine, slot: i32, state: *mut i32) -> rwkv_status;
    // `Formatter` for nested constraints: byte automata with a return-state stack (JSON), masked and committed on the device
    pub fn rwkv_pda_from_table(next: *const u16, act: *const u16, accepting: *const u8, n_states: i32, start: i32, max_depth: i32,
                               out: *mut *mut rwkv_pda) -> rwkv_status;
    pub fn rwkv_pda_json(flags: u32, max_depth: i32, out: *mut *mut rwkv_pda) -> rwkv_status;
    pub fn rwkv_pda_free(p: *mut rwkv_pda);
    pub fn rwkv_pda_num_states(p: *const rwkv_pda) -> i32;
    pub fn rwkv_pda_start(p: *const rwkv_pda) -> i32;
    pub fn rwkv_pda_max_depth(p: *const rwkv_pda) -> i32;
    pub fn rwkv_pda_table(p: *const rwkv_pda, next: *mut u16, act: *mut u16, accepting: *mut u8) -> rwkv_status;
    pub fn rwkv_pda_walk(p: *const rwkv_pda, state: i32, stack: *const u16, depth: i32, bytes: *const u8, n: usize, state_out: *mut i32,
                         stack_out: *mut u16, depth_out: *mut i32) -> rwkv_status;
    pub fn rwkv_pda_allow(p: *const rwkv_pda, state: i32, stack: *const u16, depth: i32, bytes: *const u8, lens: *const i32, n_tokens: usize,
                          allow: *mut u8, num_vocab: usize) -> rwkv_status;
    pub fn rwkv_pda_check_live(p: *const rwkv_pda, state: i32, stack: *const u16, depth: i32, lens: *const i32, bytes: *const u8,
                               n_tokens: usize) -> rwkv_status;
    pub fn rwkv_gen_set_pda(e: *mut rwkv_engine, slot: i32, pda: *const rwkv_pda, state: i32, stack: *const u16, depth: i32,
                            halt_mode: i32) -> rwkv_status;
    pub fn rwkv_gen_pda_config(e: *mut rwkv_engine, slot: i32, state: *mut i32, stack: *mut u16, cap: usize, depth: *mut i32) -> rwkv_status;
    // Tokenizer  (lib.rs:375, run.rs:157, 856, bnf.rs:15)
    pub fn rwkv_tokenizer_create(vocab_json: *const c_char, len: usize, out: *mut *mut rwkv_tokenizer) -> rwkv_status;
    pub fn rwkv_tokenizer_destroy(t: *mut rwkv_tokenizer);
    pub fn rwkv_tokenizer_encode(t: *const rwkv_tokenizer, text: *const u8, len: usize, out: *mut u32, cap: usize) -> i64;
    pub fn rwkv_tokenizer_decode(t: *const rwkv_tokenizer, tokens: *const u32, n: usize, out: *mut u8, cap: usize) -> i64;
    pub fn rwkv_tokenizer_token_bytes(t: *const rwkv_tokenizer, token: u32, out: *mut u8, cap: usize) -> i64;
    pub fn rwkv_tokenizer_vocab_size(t: *const rwkv_tokenizer) -> i64;
    // measurement hooks (bench.py / scripts; no reference counterpart)
    pub fn rwkv_profile_family_name(family: i32) -> *const c_char;
    pub fn rwkv_profile_infer(e: *mut rwkv_engine, inp: *const rwkv_slot_input, out: *mut rwkv_slot_output,
                              ms: *mut c_float, launches: *mut i32) -> rwkv_status;
    pub fn rwkv_decode_greedy(e: *mut rwkv_engine, n_slots: i32, first_tokens: *const u32, n_steps: i32,
                              out_tokens: *mut u32, elapsed_ms: *mut c_float) -> rwkv_status;
    pub fn rwkv_bench_gemm(rows: i32, k: i32, fmt: i32, t: i32, hilo: i32, ksw: i32, nmat: i32, iters: i32,
                           us_per_launch: *mut c_float, lds_kib: *mut c_float) -> rwkv_status;
}
