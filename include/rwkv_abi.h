/*
 * rwkv_abi.h — flat C ABI of librwkv_hip.so, the MI355X-native replacement for the
 * `web-rwkv` surface that ai00-core binds (ai00_server @ 2025-10-24).
 *
 * Every entry point names the reference call site it replaces (paths relative to the
 * reference root, crates/ai00-core/src/...).  Conventions:
 *   - plain pointers + sizes only; no C++/torch types cross this boundary;
 *   - every function returning `rwkv_status` returns 0 on success and a negative code on
 *     failure; `rwkv_last_error()` gives a thread-local message.  Nothing aborts — mirrors
 *     the `Result<_, RuntimeError|TensorError>` + `anyhow ?` convention (run.rs:1143);
 *   - threading contract (run.rs:1072-1190): per engine exactly two long-lived caller threads:
 *     the `infer` task (serialises rwkv_infer + all rwkv_state_* calls) and the `softmax`
 *     task (rwkv_softmax, own stream).  Tokenizer handles are immutable and thread-safe.
 *   - the library REQUIRES a gfx950 device: there is no CPU fallback; engine creation fails
 *     with RWKV_ERR_DEVICE when no HIP device is present.
 */
#ifndef RWKV_ABI_H
#define RWKV_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RWKV_ABI_VERSION 9   /* 2: rwkv_sample_params gained kind/tau; rwkv_engine_save_prefab
                              * 3: rwkv_sample_params gained allow (formatter mask); rwkv_host_alloc/free; RWKV_OPTION_NONE
                              * 4: rwkv_engine_token_chunk_size
                              * 5: rwkv_state_back_layer_async / rwkv_state_sync
                              * 6: no new symbol — rwkv_infer no longer waits for a step that emits no row; rwkv_state_back_layer_async checks
                              *    that the rows end inside the pinned block that holds `dst`
                              * 7: rwkv_load_desc.precision: RWKV_PRECISION_FP16 now holds 1e-3 at depth (the launches that carry a model's f16 operand
                              *    rounding read hi + lo operands); the old all-f16 behaviour is RWKV_PRECISION_FP16_RAW
                              * 8: device-resident sampled generation: rwkv_gen_params, rwkv_gen_arm / _disarm / _run, rwkv_gen_uniform
                              * 9: resident generation admits prompts: rwkv_gen_arm_prompt (prefill rides in the resident steps, the first token is drawn
                              *    on the device), rwkv_gen_prompt_left
                              *    additive under 9 (no existing symbol or struct changed): rwkv_infer_score, rwkv_score_rows, RWKV_SCORE_SKIP: target tokens
                              *    are scored on the device, 4 bytes per token come back instead of a logits row
                              *    additive under 9: rwkv_gen_set_token_bytes, rwkv_gen_set_stops, rwkv_gen_stop_tail, RWKV_GEN_HANDBACK: stop STRINGS are
                              *    matched on the device inside the resident step
                              *    additive under 9 (no new symbol, no struct changed): RWKV_V4 — RWKV-4 World checkpoints load (version 4 in
                              *    rwkv_model_info, the five-row state below); they were RWKV_ERR_UNSUPPORTED before
                              *    additive under 9: rwkv_dfa_* (byte automata, host only), rwkv_gen_set_constraint, rwkv_gen_constraint_state: a REGULAR
                              *    format constraint is masked and advanced on the device inside the resident step
                              *    additive under 9: rwkv_topn_rows, rwkv_infer_topn, rwkv_gen_set_topn, rwkv_gen_run_topn, RWKV_TOPN_MAX, RWKV_TOPN_NONE: the
                              *    n most likely tokens of a row and their ln-probabilities are listed on the device (host rows, prefill, resident
                              *    generation), 8 n bytes per row come back instead of the row
                              *    additive under 9: rwkv_pda_* (byte automata with a return-state stack, host only; rwkv_pda_json is RFC 8259),
                              *    rwkv_gen_set_pda, rwkv_gen_pda_config: a NESTED format constraint ("answer in JSON") is masked and advanced on the
                              *    device inside the resident step
                              *    additive under 9: rwkv_gen_watch_open / _close / _head / _read / _cancel, RWKV_GEN_CANCELLED, RWKV_GEN_WATCH_MAX_STEPS:
                              *    another thread streams the tokens of a running rwkv_gen_run and cancels slots inside it
                              *    additive under 9: rwkv_gen_set_capture, rwkv_gen_take_item, rwkv_gen_item_free / _state / _back / _from_host,
                              *    rwkv_gen_arm_item, RWKV_GEN_CAPTURE_PROMPT / _FINISH: resident generation fills the prefix cache (the state and raw
                              *    row at the prompt's end and at a stop) and arms a slot from a cached item
                              *    additive under 9 (no new symbol, no struct changed): RWKV_QUANT_SF4 — `Quant::SF4` models load: NF4's storage read
                              *    through the Student-t code book; rwkv_bench_gemm takes fmt 3 */

typedef int32_t rwkv_status;
enum {
    RWKV_OK = 0,
    RWKV_ERR_INVALID = -1,     /* bad argument / malformed input            */
    RWKV_ERR_FORMAT = -2,      /* not a safetensors file / missing tensor   */
    RWKV_ERR_UNSUPPORTED = -3, /* model version (v5.0/5.1, unknown naming), dimensions or option */
    RWKV_ERR_DEVICE = -4,      /* no HIP device / HIP runtime error         */
    RWKV_ERR_OOM = -5,
    RWKV_ERR_NO_STATE = -6     /* file has no `time_state` tensors (lib.rs:442) */
};

/* thread-local text of the last failure on this thread ("" if none). */
const char *rwkv_last_error(void);
int32_t rwkv_abi_version(void);

/* ---- adapters: `list_adapters` lib.rs:339-349, surfaced by /api/adapters (adapter.rs:8-14) */
int32_t rwkv_device_count(void);
rwkv_status rwkv_device_name(int32_t index, char *buf, size_t buf_len);

/* ---- `Loader::info(&SafeTensors)` lib.rs:587, api/file.rs:113-116 -> `ModelInfo` ---------- */
enum { RWKV_V4 = 4, RWKV_V5 = 5, RWKV_V6 = 6, RWKV_V7 = 7 };
/* V4 is detected on positive evidence only: blocks.0 has none of att.ln_x.weight / att.gate.weight / att.time_mix_x / att.x_r, has
 * att.time_first and att.time_decay with exactly num_emb elements, and att.time_mix_k/v/r and ffn.time_mix_k/r; anything else that is not
 * V5.2 / V6 / V7 stays RWKV_ERR_UNSUPPORTED.  V4 has no heads: num_head = 1, head_size = num_emb.  The dimension rules (num_emb % 64,
 * num_hidden % 32, num_vocab % 16 == 0) hold for every version, so the 50277-token Pile models of RWKV-4 are refused here as the World
 * tokenizer refuses them; the RWKV-4 World models (65536 tokens) load. */
typedef struct rwkv_model_info {
    int32_t version;     /* ModelVersion: 4, 5 (=v5.2), 6, 7 */
    int32_t num_layer;
    int32_t num_emb;
    int32_t num_hidden;
    int32_t num_vocab;
    int32_t num_head;
    int32_t head_size;   /* num_emb / num_head (64; V4: num_emb) */
    int32_t reserved;
} rwkv_model_info;
rwkv_status rwkv_model_info_from_st(const uint8_t *st_bytes, size_t st_len, rwkv_model_info *out);
/* `st_bytes` here and in rwkv_load_desc may also be a PREFAB image written by rwkv_engine_save_prefab: the content is
 * sniffed exactly as lib.rs:585-588 does (safetensors, else prefab).  A prefab carries the re-tiled / quantised /
 * LoRA-blended weights, so loading it skips those passes; its quantisation settings override the descriptor's and
 * LoRA adapters are rejected (RWKV_ERR_UNSUPPORTED).  The format is this library's own (versioned), not web-rwkv's CBOR. */

/* ---- `create_context` lib.rs:351-368 + `load_runtime` lib.rs:391-516 ---------------------- */
/* `Quant` lib.rs:689-704, all four values.  The formats are this library's own (web-rwkv's layouts and tables cannot be read here):
 * INT8 128-element blocks {a, b}; NF4 and SF4 64-element blocks, fp16 absmax, a 16-entry code book — NF4's the normal quantiles of
 * QLoRA, SF4's the same construction over Student's t with 5 degrees of freedom (Dotzel et al. 2024).  Any other value: RWKV_ERR_UNSUPPORTED. */
enum { RWKV_QUANT_NONE = 0, RWKV_QUANT_INT8 = 1, RWKV_QUANT_NF4 = 2, RWKV_QUANT_SF4 = 3 };
/* `Precision` reload.rs:89-94, passed by `load_runtime` lib.rs:503-515.  GEMM operands are f16 with fp32 accumulation in every mode:
 *   FP16 (the reference's default, and this library's): f16 operands, except that the launches whose input rounding carries a model's
 *        error at depth read the operand as a hi + lo f16 pair (V5 / V6: the time-mix projections and first-stage LoRAs; V7: those, the
 *        second-stage LoRAs and the output projection) — logits, state and embeddings within 1e-3 of an fp32 evaluation at 32 layers;
 *   FP32: every launch reads hi + lo operands (fp32-class: <= 2e-5);
 *   FP16_RAW: f16 operands everywhere — the fastest mode; relative error ~1e-3 of the row's magnitude, NOT within 1e-3 absolute at 32 layers
 *        (V7-2.9B NF4 measures 4.7e-3).  For callers that accept that.
 * Saturation, in every mode: an activation outside f16's range enters a matrix product as +-65504 (operands saturate); no operand
 * becomes inf or NaN.  This is about activations; a quantised weight is whatever its format dequantises to. */
enum { RWKV_PRECISION_FP16 = 0, RWKV_PRECISION_FP32 = 1, RWKV_PRECISION_FP16_RAW = 2 };
enum { RWKV_ADAPTER_AUTO = -1, RWKV_ADAPTER_ECONOMICAL = -2 };           /* reload.rs AdapterOption; >=0 = Manual(n) */

typedef struct rwkv_lora_desc {    /* `reload::Lora{path, alpha}` + LoraBlend::full(alpha), lib.rs:466-482 */
    const uint8_t *st_bytes;
    size_t st_len;
    float alpha;
} rwkv_lora_desc;

typedef struct rwkv_load_desc {    /* the `ReloadRequest` fields that reach web-rwkv, lib.rs:200-231 */
    int32_t adapter;               /* RWKV_ADAPTER_* or device index (Manual(n))            */
    int32_t quant_layers;          /* `quant`: layers 0..quant are quantised (lib.rs:465)   */
    int32_t quant_type;            /* RWKV_QUANT_*                                          */
    int32_t precision;             /* RWKV_PRECISION_*: activation precision at GEMM inputs */
    int32_t max_batch;             /* state slots resident on the device (default 8)        */
    int32_t token_chunk_size;      /* max tokens consumed per rwkv_infer call (default 128) */
    const uint8_t *st_bytes;       /* model `.st` bytes (caller's mmap; released after return, lib.rs:446) */
    size_t st_len;
    const rwkv_lora_desc *lora;    /* may be NULL */
    size_t n_lora;
} rwkv_load_desc;

typedef struct rwkv_engine rwkv_engine;   /* = Context + Model + vN::Bundle + TokioRuntime<Rnn> + State */

rwkv_status rwkv_engine_create(const rwkv_load_desc *desc, rwkv_engine **out);
void rwkv_engine_destroy(rwkv_engine *e);                       /* Unload/drop lib.rs:652-656 */
/* `ModelSerialize::serialize(file)` lib.rs:131-154 (the "save model" admin call): write the loaded model as a prefab image. */
rwkv_status rwkv_engine_save_prefab(rwkv_engine *e, const char *path);
rwkv_status rwkv_engine_info(const rwkv_engine *e, rwkv_model_info *out);
int32_t rwkv_engine_device(const rwkv_engine *e);               /* HIP device ordinal in use */
int32_t rwkv_engine_max_batch(const rwkv_engine *e);
int32_t rwkv_engine_token_chunk_size(const rwkv_engine *e);     /* the load-time `token_chunk_size` (lib.rs:221-223): rows one rwkv_infer call emits at most per Full slot */
/* bytes of weights resident in HBM at their storage width (fp16 / int8+scales / nf4 or sf4+absmax),
 * embedding table excluded: the W_q of SURVEY 8(d).  For roofline accounting. */
uint64_t rwkv_engine_weight_bytes(const rwkv_engine *e);

/* ---- `runtime.infer(RnnInput) -> (RnnInput, RnnOutput)` run.rs:1134-1156 ------------------ */
enum { RWKV_OPTION_LAST = 0, RWKV_OPTION_FULL = 1,              /* RnnOption, run.rs:716,819 */
       RWKV_OPTION_NONE = 2 };   /* extension: consume the tokens, emit no row (state-only jobs: the documented `/embeddings`
                                  * route, docs/doc-api/openai.md:376-437, reads back a state slice and never looks at logits);
                                  * a step in which no slot emits skips the final LayerNorm, the head GEMM and the logits copy */
typedef struct rwkv_slot_input {   /* RnnInputBatch::new(tokens, option) run.rs:1128 */
    const uint32_t *tokens;        /* remaining tokens of this slot (may be NULL if n_tokens==0) */
    size_t n_tokens;
    int32_t option;                /* RWKV_OPTION_* */
    int32_t reserved;
} rwkv_slot_input;
typedef struct rwkv_slot_output {  /* RnnOutputBatch, run.rs:1146-1155 */
    float *logits;                 /* caller buffer, >= logits_capacity_rows * num_vocab floats */
    size_t logits_capacity_rows;
    size_t n_rows;                 /* OUT: rows written (0 = nothing emitted this call)      */
    size_t n_consumed;             /* OUT: tokens of this slot consumed by this call          */
} rwkv_slot_output;
/* One forward step over <= token_chunk_size tokens spread across the `max_batch` slots
 * (arrays have max_batch entries).  The caller advances `tokens` by `n_consumed` and calls
 * again while any tokens remain (the `while input.num_token() > 0` loop, run.rs:1134).
 * Last: one row when the slot's tokens are exhausted by this call.  Full: one row per token
 * consumed.  State of each touched slot is updated in place on the device.  A call that emits rows returns when they are in the
 * caller's buffers.  A call that emits NO row (state-only slots, or `Last` slots whose tokens are not exhausted yet) returns as soon as
 * the step is queued: `n_consumed` is final, the device runs behind, and everything that reads device data afterwards (a later
 * rwkv_infer with rows, rwkv_state_back / _read / _write / _back_layer[_async]) is ordered behind it — host work between two steps of a
 * long prefill overlaps the device.  The `tokens` arrays may be reused as soon as the call returns (they are staged on return).  Errors of such a
 * call: a launch error is returned by the call itself; an asynchronous device fault of the queued step is returned by the NEXT call that waits
 * (a step with rows, rwkv_state_back / _read / _sync), and the states of the slots the step touched are undefined from then on. */
rwkv_status rwkv_infer(rwkv_engine *e, const rwkv_slot_input *in, rwkv_slot_output *out);

/* Pinned host memory for the `logits` buffers of rwkv_infer (the `TensorCpu<f32>` outputs of run.rs:1146-1155 are read back
 * through mapped staging buffers in web-rwkv; this is the equivalent on the HIP side).  When every destination of a call is
 * pinned, rows are copied device-to-host straight into it (destinations contiguous in slot order become one copy: hand the
 * slots consecutive pieces of one block); pageable buffers still work and take a staged copy.  Any thread; free with
 * rwkv_host_free. */
rwkv_status rwkv_host_alloc(size_t bytes, void **out);
void rwkv_host_free(void *p);

/* The chunk policy of rwkv_infer as a pure host function (no device needed): how many of each slot's pending tokens one
 * call consumes — water-filling of `token_chunk_size`, so decode slots are never starved by a long prefill
 * (web-rwkv's own split inside `RnnInput::new(batches, chunk)` run.rs:1132 is not visible; any split is
 * result-equivalent). */
rwkv_status rwkv_plan_chunk(int32_t max_batch, int32_t token_chunk_size, const size_t *n_tokens, int32_t *consumed);

/* ---- `State` trait: run.rs:477,950 (init) 1099 (load) 1101 (back) 1104 (write) 1106 (read) -- */
size_t rwkv_state_len(const rwkv_engine *e);                       /* floats in one slab      */
void rwkv_state_shape(const rwkv_engine *e, size_t shape[4]);      /* [C, N+2, L, 1] run.rs:987; V4: [C, 5L, 1, 1] */
rwkv_status rwkv_state_init(const rwkv_engine *e, float *dst);     /* zero slab (CPU); V4: see below */
/* V4 state: 5L rows of C floats, layer l owns rows 5l .. 5l+4 = time-mix shift, aa, bb, pp, channel-mix shift (aa / bb: numerator and
 * denominator of the WKV average, pp: their common exponent).  rwkv_state_init writes 0 everywhere and -1e30 in the pp rows.
 * [EXT] The row order and the init constant are web-rwkv's (its V4 state is [C, 5L, 1]; the crate is not vendored in the reference
 * tree, so neither can be checked against it here).  The kernels give the same bits for pp = -1e30 and pp = -FLT_MAX. */
rwkv_status rwkv_state_load(rwkv_engine *e, int32_t slot, const float *src);   /* H2D         */
rwkv_status rwkv_state_back(rwkv_engine *e, int32_t slot, float *dst);         /* D2H, blocks */
typedef struct rwkv_dstate rwkv_dstate;                            /* TensorGpu snapshot       */
rwkv_status rwkv_state_read(rwkv_engine *e, int32_t slot, rwkv_dstate **snap); /* D2D copy out */
rwkv_status rwkv_state_write(rwkv_engine *e, int32_t slot, const rwkv_dstate *snap); /* D2D in; snap reusable */
void rwkv_dstate_free(rwkv_dstate *snap);
/* f-2 (docs/doc-api/openai.md:376-437): one layer's WKV rows [N][C] of a slot, D2H (V4: its aa, bb, pp rows [3][C]) */
rwkv_status rwkv_state_back_layer(rwkv_engine *e, int32_t slot, int32_t layer, float *dst);
/* The same read-back, NOT waited for: the layer's rows are packed on a second stream (ordered behind everything issued so far; later
 * work on the slot — rwkv_infer, rwkv_state_load / _write — is ordered behind the pack, a few microseconds) and copied to `dst`, which
 * must be pinned host memory (rwkv_host_alloc), while the engine goes on with the next rwkv_infer.  An embedding job (`/embeddings`,
 * docs/doc-api/openai.md:376-437; the reference's `state.back(batch).await` yields to the other tasks the same way, run.rs:1101) hands a
 * finished document's slot to the next document without waiting for PCIe.  `dst` is valid after rwkv_state_sync. */
rwkv_status rwkv_state_back_layer_async(rwkv_engine *e, int32_t slot, int32_t layer, float *dst);
rwkv_status rwkv_state_sync(rwkv_engine *e);                       /* wait for every pending rwkv_state_back_layer_async */

/* ---- `vN::read_state(context, info, model)` lib.rs:378-389 ---------------------------------
 * On a V4 engine: RWKV_ERR_UNSUPPORTED, as the reference bails ("v4 does not support init state yet", lib.rs:384). */
rwkv_status rwkv_read_init_state(const rwkv_engine *e, const uint8_t *st_bytes, size_t st_len, float *dst);

/* ---- `softmax::softmax(&context, Vec<TensorCpu>)` run.rs:1178-1183 -------------------------
 * n rows of num_vocab floats each, host pointers in / out (may alias).  Own stream: may run
 * concurrently with rwkv_infer from the second caller thread. */
rwkv_status rwkv_softmax(rwkv_engine *e, const float *const *in, float *const *out, size_t n_rows);

/* ---- scoring on the device: what `perplexity` (run.rs:699-755) and GenerateKind::Choose (run.rs:936-982) need of a logits row is ONE
 * number, the probability the model gave to the token that actually followed.  Both calls return its natural logarithm
 *      logp = (x[t] - m) - ln sum_i exp(x[i] - m),   m = max_i x[i]
 * computed on the device in one pass over the row (fp32, a fixed reduction order: a row's result depends on its bits, its target and num_vocab only,
 * not on how many rows ride along), within 2e-5 * max(1, |logp|) of a float64 evaluation.
 *  - DEVIATION from the reference, on purpose: run.rs:737-740 exponentiates WITHOUT subtracting the maximum, so it yields inf / NaN once a logit
 *    passes about 88; this form stays finite there.  Wherever the reference is finite the two agree to the bound above.
 *  - target RWKV_SCORE_SKIP: the row is not scored, the output is a quiet NaN (the last row of a perplexity request has no next token).
 *  - x[t] == -inf (a masked token) gives -inf, not NaN; a row holding +inf or NaN gives NaN.
 *  - any other target >= num_vocab: RWKV_ERR_INVALID before anything is launched or written. */
#define RWKV_SCORE_SKIP 4294967295u   /* 0xFFFFFFFF */
/* like rwkv_softmax: n_rows host rows of num_vocab floats in, one ln-probability per row out; own (softmax) stream and the softmax task's thread.
 * This is Choose's `head` term (the probability of choice[0] on the prompt's last row, run.rs:971-972) when the caller holds the row. */
rwkv_status rwkv_score_rows(rwkv_engine *e, const float *const *in, const uint32_t *targets, float *out_logp, size_t n_rows);
/* like rwkv_infer, for slots that are scored instead of read.  All arrays have max_batch entries.  A slot with targets[b] != NULL is SCORED: it
 * is planned as RWKV_OPTION_FULL (in[b].option is ignored; the rwkv_plan_chunk split and the step shapes are those of rwkv_infer, so the rows that are
 * scored are the very rows a Full call with the same occupancy would have returned), targets[b] has in[b].n_tokens entries, targets[b][i] is scored
 * on the row produced by consuming tokens[b][i], and out_logp[b][0 .. n_consumed[b]) is written by this call; the caller advances tokens, targets
 * and out_logp together by n_consumed[b].  A slot with targets[b] == NULL must have n_tokens == 0 or option == RWKV_OPTION_NONE (a state-only
 * prefill riding along), else RWKV_ERR_INVALID.  No logits row crosses PCIe: 4 bytes per row do.  The call returns when the scores are in place (a
 * call in which only state-only slots ride returns when the step is queued, as rwkv_infer does); errors as for a row-emitting rwkv_infer.  Thread
 * contract of rwkv_infer; tokens for an armed generation slot disarm it. */
rwkv_status rwkv_infer_score(rwkv_engine *e, const rwkv_slot_input *in, const uint32_t *const *targets, float *const *out_logp, size_t *n_consumed);

/* ---- top-n lists on the device: what the `top_logprobs` of a completion, a classifier over a few label tokens or a per-token
 * uncertainty estimate need of a logits row is the n most likely tokens and their ln-probabilities.  For a row x[0 .. num_vocab) and
 * 1 <= n <= RWKV_TOPN_MAX a LIST is n (id, logp) pairs:
 *  - order: the entries with x[i] > -inf, by x[i] descending as real numbers (-0 equals +0), ties to the lower token id.  The ids are a function
 *    of the row's bits alone: two different logits never tie, even where their probabilities round to one float or underflow to zero.
 *  - logp is rwkv_score_rows' value for that row with that id as target, bit for bit (the same reduction in the same order).
 *  - fewer than n such entries (masked tokens, n > num_vocab, a row of nothing but -inf): the places left hold (RWKV_TOPN_NONE, -inf).
 *  - a row holding +inf or NaN: all n places hold (RWKV_TOPN_NONE, NaN), as rwkv_score_rows gives NaN.
 *  - a row's list does not depend on how many rows ride along.
 * n outside 1 .. RWKV_TOPN_MAX or a null pointer: RWKV_ERR_INVALID before anything is launched or written.
 * rwkv_infer_sample returns no lists: a caller that samples token by token and wants them takes the row (rwkv_infer) and lists it with
 * rwkv_topn_rows. */
#define RWKV_TOPN_MAX 32
#define RWKV_TOPN_NONE 4294967295u   /* 0xFFFFFFFF */
/* like rwkv_score_rows: n_rows host rows of num_vocab floats in, out_ids / out_logp [n_rows][n] out; own (softmax) stream and the softmax task's
 * thread; staged in pieces of max_batch rows. */
rwkv_status rwkv_topn_rows(rwkv_engine *e, const float *const *in, int32_t n, uint32_t *out_ids, float *out_logp, size_t n_rows);
/* rwkv_infer with lists instead of rows.  All arrays have max_batch entries.  A slot with out_ids[b] != NULL keeps its option: RWKV_OPTION_LAST
 * lists the one row of the call that exhausts its tokens, RWKV_OPTION_FULL one row per consumed token; out_ids[b] / out_logp[b] take [rows][n]
 * entries (room for 1 resp. n_tokens rows) and n_rows[b] says how many lists this call wrote.  The plan, the rwkv_plan_chunk split and the step
 * shapes are rwkv_infer's: the rows listed are the very rows rwkv_infer would have returned at the same occupancy.  A slot with out_ids[b] ==
 * NULL must have n_tokens == 0 or option == RWKV_OPTION_NONE, else RWKV_ERR_INVALID.
 * `targets` may be NULL as a whole or per slot.  Where targets[b] is given the slot must be RWKV_OPTION_FULL and listing; targets[b] has
 * n_tokens entries (token ids or RWKV_SCORE_SKIP) and out_tok_logp[b][i] is exactly rwkv_infer_score's value for that row: the realised token's
 * ln-probability beside the alternatives, in one pass (`echo`).  The caller advances tokens, targets and the outputs by n_consumed[b].
 * No logits row crosses PCIe.  Returns when the lists are in place (a call in which no slot reaches a row returns when the step is queued, as
 * rwkv_infer does); errors, thread contract and disarming rule of rwkv_infer. */
rwkv_status rwkv_infer_topn(rwkv_engine *e, const rwkv_slot_input *in, int32_t n, uint32_t *const *out_ids, float *const *out_logp,
                            const uint32_t *const *targets, float *const *out_tok_logp, size_t *n_rows, size_t *n_consumed);

/* ---- on-device sampling front-end: what `sample()` run.rs:664-697 + NucleusSampler::sample
 * (sampler/nucleus.rs:69-101) do with three PCIe hops and a 65,536-element CPU sort, done on the device.
 * The caller keeps the sampler STATE (penalty map, nucleus.rs:104-119) and passes its effect as sparse logit
 * adjustments (-penalty[token] + bias[token], duplicates merged) plus the uniform draw `fastrand::f32()` would make. */
typedef struct rwkv_sample_params {
    float top_p;                   /* NucleusParams defaults: 0.5 / 128 / 1.0 (nucleus.rs:13-26) */
    int32_t top_k;                 /* any value: above num_vocab it is num_vocab, below 1 nothing is kept and the token is 0.  The candidates */
                                   /*   are ordered by key descending, TIES TO THE LOWER TOKEN ID (the reference's sort is unstable); tokens  */
                                   /*   of probability 0 are never candidates.  top_k <= 256 runs the narrow kernel, above it the wide one.  */
    float temperature;
    float uniform;                 /* u in [0,1) */
    const uint32_t *adj_tokens;    /* may be NULL when n_adj == 0 */
    const float *adj_values;       /* added to logits[adj_tokens[i]] before the softmax */
    size_t n_adj;
    int32_t kind;                  /* RWKV_SAMPLER_NUCLEUS: top_p / top_k / temperature (nucleus.rs:69-101).                 */
    float tau;                     /* RWKV_SAMPLER_TYPICAL (typical.rs:70-120; defaults 0.5 / 128 / 1.0): keys |(-ln p) - H|  */
                                   /*   ascending, take top_k, keep while the cumulative probability before an element <= tau */
                                   /* RWKV_SAMPLER_MIROSTAT (mirostat.rs:44-90): tau = the sampler's current `max_surprise`;  */
                                   /*   top_p / top_k / temperature unused; out_probs[b] returns the TOKEN SURPRISE           */
                                   /*   log2(sum) - log2(p) the caller needs for `max_surprise -= rate * (surprise - tau)`.   */
                                   /*   Exact for every max_surprise: below 13 (fewer than 8192 candidates can qualify) the narrow kernel    */
                                   /*   holds them all, from 13 on the wide one walks the sorted row in windows of 8192.  BIT RULE: on a row */
                                   /*   both kernels can hold, the wide one returns the narrow one's token and out_probs bits.              */
    const uint8_t *allow;          /* NULL, or num_vocab bytes: allow[token] == 0 forbids the token (its logit becomes -inf before  */
                                   /*   the softmax).  This is what a `Formatter::transform` leaves behind (run.rs:676-679,         */
                                   /*   sampler/bnf.rs:35-38: kbnf's mask_logits): the grammar state machine stays on the host and  */
                                   /*   hands over its current allowed-token set, so BNF-constrained requests can sample on the     */
                                   /*   device too.                                                                                 */
} rwkv_sample_params;
enum { RWKV_SAMPLER_NUCLEUS = 0, RWKV_SAMPLER_TYPICAL = 1, RWKV_SAMPLER_MIROSTAT = 2 };
/* Like rwkv_infer with RWKV_OPTION_LAST on every slot, but slots whose pending tokens are exhausted by this call
 * get a sampled token id (out_tokens[b], emitted[b] = 1, out_probs[b] = its softmax probability) instead of a
 * logits row; only 8 bytes per slot cross PCIe.  n_consumed[b] as in rwkv_slot_output.  num_vocab <= 65536. */
rwkv_status rwkv_infer_sample(rwkv_engine *e, const rwkv_slot_input *in, const rwkv_sample_params *sp,
                              uint32_t *out_tokens, float *out_probs, uint8_t *emitted, size_t *n_consumed);

/* ---- device-resident sampled generation (completed): the decode loop of `process` (run.rs:788-1020) with `sample()`
 * (run.rs:664-697) and the whole `Sampler` state machine (sampler/nucleus.rs, typical.rs, mirostat.rs) kept on the device.  A slot is
 * ARMED with its sampler settings; rwkv_gen_run then generates up to n_steps tokens per armed slot with one captured graph launch per
 * step and no host turn-around between tokens; only token ids and probabilities cross PCIe.
 *
 *  - Sampler arithmetic is that of the per-token path (rwkv_infer_sample fed by include/rwkv_sampler.hpp), bit for bit: a token with
 *    penalty p and bias b gets  x + ((-p) + b)  (transform nucleus.rs:61-67, then the bias loop run.rs:681-683, merged in that order),
 *    then the same sampling kernel runs.  After the draw every PRESENT penalty is multiplied by penalty_decay and the drawn token's entry
 *    becomes presence_penalty if it was absent, else entry + frequency_penalty (nucleus.rs:104-119).  Absent is membership, not value:
 *    with presence_penalty = 0 the entry exists after the first draw.  Mirostat: max_surprise = fmin(max_surprise - rate * (surprise -
 *    target), 4 * target) (mirostat.rs:85-87), each operation rounded to f32 on its own (no fused multiply-add).
 *  - The uniform draw `fastrand::f32()` would make (nucleus.rs:93) is a counter function, so that a host can restate any step:
 *        z = seed + 0x9E3779B97F4A7C15 * (((uint64)stream << 32 | step) + 1)        (mod 2^64)
 *        z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *        u = (float)(z >> 40) * 2^-24                                               exact in f32, in [0, 1)
 *    `step` counts the draws of the slot since rwkv_gen_arm and carries over from one rwkv_gen_run to the next.
 *  - STATE RULE: when rwkv_gen_run returns, a slot's state has consumed `first_token` and every token emitted so far EXCEPT THE LAST ONE
 *    EMITTED — whether the slot is still running (the last token is held on the device; the next run continues from it), hit a stop
 *    token, or reached max_tokens.  That is the state the reference backs up at a stop (run.rs:990-1005).  A stop token is emitted as the
 *    slot's last token.  Token 0 always stops (run.rs:855).
 *  - A slot that finishes inside a run keeps riding the remaining steps of that run (the captured step does not change shape); its rows
 *    are computed and thrown away and its state is put back as the rule says before the call returns.  It takes no part in later runs.
 *  - Stop STRINGS (`GenerateRequest::stop`, run.rs:899-932) are matched on the device, inside the step, over the decoded bytes of the
 *    output: rwkv_gen_set_token_bytes hands the engine what `tokenizer.decode(&[token])` yields per id, rwkv_gen_set_stops hands an armed
 *    slot its strings.  The matcher is the reference's, byte for byte — per drawn token the whole buffer is walked once per string, the
 *    mismatching byte is not retried as a new start ("ab" over "aab" does not match), `min_by` picks a matched string before an unmatched
 *    one and then the smallest index, and the part in front of that index leaves the buffer only when it is valid UTF-8 (run.rs:1008-1010)
 *    — so a slot finishes with RWKV_GEN_STOP at the token the reference stops at, with the state the rule above prescribes, whatever
 *    n_steps is.  An id that is not in the table is the reference's decode error: empty word, stop (run.rs:856-862).  A slot without
 *    strings runs what it ran before.  When a token's bytes do not fit the slot's RWKV_GEN_STOP_BUF bytes of buffer (a head that never
 *    becomes valid UTF-8 keeps growing) the slot finishes with RWKV_GEN_HANDBACK: the token is emitted and the state rule holds as for any
 *    finish; the caller, who has every token, replays its own matcher (include/rwkv_scheduler.hpp StopMatcher) and goes on per token.
 *    A slot that finishes — whatever the reason — leaves its buffer as it was before its last token.
 *  - FORMAT CONSTRAINTS: a formatter that needs the host between two tokens — kbnf's context-free grammars, sampler/bnf.rs — stays
 *    refused here; what this mode offers instead is a byte-level DFA (rwkv_dfa_*, rwkv_gen_set_constraint below), masked and advanced on
 *    the device, and a byte automaton with a return-state stack (rwkv_pda_*, rwkv_gen_set_pda below) for nesting, JSON above all.  They
 *    are a second and a third implementation of the `Formatter` trait (bnf.rs:34-48), for REGULAR constraints and for what a return-state
 *    stack expresses; neither is kbnf or a port of it, and context-free grammars beyond that keep the per-token path.
 *  - Not available in this mode (RWKV_ERR_UNSUPPORTED from rwkv_gen_arm): a host-computed formatter mask (`allow` must be NULL,
 *    run.rs:676-679 — keep using rwkv_infer_sample for a grammar), top_k > 256 (Nucleus / Typical) unless `reserved` carries
 *    RWKV_GEN_WIDE_TOP_K, more than RWKV_GEN_MAX_STOP stop tokens, num_vocab > 65536.
 *  - RWKV_GEN_WIDE_TOP_K (bit 0 of `reserved`; the other bits are ignored) arms Nucleus / Typical with any top_k (above num_vocab:
 *    num_vocab); the slot then takes the wide kernel iff top_k > 256.  Mirostat needs no flag: a slot whose max_surprise can reach 13
 *    (max(tau, 4 * miro_target) >= 13) takes the wide kernel for its whole life, and by the bit rule (rwkv_sample_params) it emits what
 *    the per-token path emits, which routes by the current max_surprise.
 *  - rwkv_infer on OTHER slots between two runs is allowed (continuous batching: prefill a new request, arm it, carry on).  rwkv_infer /
 *    rwkv_infer_sample with tokens for an armed slot, rwkv_state_load and rwkv_state_write on it disarm it.
 *  Same thread contract as rwkv_infer (the `infer` task). */
#define RWKV_GEN_MAX_STOP 8
#define RWKV_GEN_MAX_STOP_STR 8   /* stop strings per slot                                  */
#define RWKV_GEN_STOP_LEN 128     /* bytes per stop string                                  */
#define RWKV_GEN_STOP_BUF 512     /* bytes of matcher buffer per slot (`context.buffer`)    */
#define RWKV_GEN_TOKEN_LEN 256    /* bytes per token of the token table                     */
#define RWKV_GEN_WIDE_TOP_K 1     /* rwkv_gen_params.reserved: top_k > 256 is armed, not refused */
typedef struct rwkv_gen_params rwkv_gen_params;
struct rwkv_gen_params {
    uint32_t first_token;          /* the token the first step consumes: the one the caller sampled from the prompt's row (run.rs:809-832)  */
    int32_t max_tokens;            /* emit at most this many, > 0 (`max_tokens`, run.rs:905-917)                                            */
    int32_t kind;                  /* RWKV_SAMPLER_*                                                                                       */
    float top_p;                   /* as in rwkv_sample_params: nucleus.rs:13-26, typical.rs:11-24                                         */
    int32_t top_k;
    float temperature;
    float tau;                     /* Typical: tau.  Mirostat: the initial max_surprise (2 * target, mirostat.rs:30-36)                     */
    float presence_penalty;        /* nucleus.rs:13-26 / typical.rs:11-24; unused by Mirostat                                               */
    float frequency_penalty;
    float penalty_decay;
    float miro_target;             /* mirostat.rs:85-87: `tau` and `rate` of MirostatParams                                                 */
    float miro_rate;
    const uint32_t *penalty_tokens; /* the penalty map `init` left over the prompt (nucleus.rs:49-59); may be NULL when n_penalty == 0      */
    const float *penalty_values;
    size_t n_penalty;
    const uint32_t *bias_tokens;   /* GenerateRequest::bias (run.rs:681-683); may be NULL when n_bias == 0                                  */
    const float *bias_values;
    size_t n_bias;
    const uint32_t *stop_tokens;   /* extra stop tokens, n_stop <= RWKV_GEN_MAX_STOP; token 0 always stops (run.rs:855)                     */
    size_t n_stop;
    const uint8_t *allow;          /* must be NULL (see above)                                                                              */
    uint64_t seed;                 /* rwkv_gen_uniform(seed, stream, step)                                                                  */
    uint32_t stream;
    uint32_t reserved;             /* RWKV_GEN_WIDE_TOP_K or 0                                                                              */
};
enum { RWKV_GEN_RUNNING = 0, RWKV_GEN_STOP = 1, RWKV_GEN_LENGTH = 2,     /* FinishReason::{Stop, Length} run.rs:905-917; 0 = not finished */
       RWKV_GEN_HANDBACK = 3 };   /* the slot's stop-string buffer is full: the device cannot decide this token, the caller goes on (see above) */
/* arm `slot` (its state is what the prompt left, run.rs:788-832); re-arming replaces the context.  The arrays are copied. */
rwkv_status rwkv_gen_arm(rwkv_engine *e, int32_t slot, const rwkv_gen_params *p);
/* Arm `slot` with a PROMPT instead of a first token (ADMISSION: the engine may be generating on other slots, nobody stands still).
 * `p->first_token` is ignored.  The penalty arrays are the map `Sampler::init` left over the prompt (nucleus.rs:49-59), i.e. BEFORE any
 * draw; the caller still computes it on the host (rwkv_sampler.hpp).  The slot's state is whatever it holds (zero, an InitState, a
 * prefix-cache hit); `tokens` are the not-yet-consumed tail of the prompt, n_tokens >= 1 (else RWKV_ERR_INVALID), copied on return.
 *  - A STEP of rwkv_gen_run then carries one feedback row per running slot plus, for every slot still in its prompt, a share of what is
 *    left of token_chunk_size after those rows — the split rwkv_plan_chunk gives with n_tokens = 1 for a running slot; decode rows come
 *    first and are never starved (there must be fewer running slots than token_chunk_size).  A prompt slot emits nothing (0xFFFFFFFF /
 *    NaN in its column) until its prompt is exhausted.
 *  - In the step that exhausts the prompt its last row is sampled on the device with draw counter step = 0 of (seed, stream), by the same
 *    arithmetic as every later draw; penalty / Mirostat update, stop-token and max_tokens tests follow as after any draw.  That token is
 *    the slot's first emitted token and counts towards max_tokens; the slot carries on as an armed slot.
 *  - STATE RULE, base case: a slot that finishes on its first draw has consumed exactly the prompt.
 *  - The refusals of rwkv_gen_arm apply.  What disarms a slot drops its pending prompt too.  A prompt may straddle rwkv_gen_run calls.
 *  - When every running slot has finished and only prompt slots remain, the run goes on until n_steps.
 *  - WHAT A JOINER DOES TO THE OTHERS: a step is bit-exact for a given number of rows whatever the neighbouring rows hold, but only
 *    2e-5 across step shapes (a one-token-per-slot step fuses LayerNorm and token shift into its GEMMs, a step that carries prompt rows
 *    does not).  While a prompt is being consumed the running slots' rows are in steps of another shape, so their logits move in the
 *    last bits (seen: 109 units in the last place of a probability, ids equal) and a draw that sits on a boundary of the cumulative
 *    distribution can pick another token: a request's output depends, at that level, on who else arrives.  It is exactly what the
 *    per-token calls give when issued with the same rows per step.
 *  - All armed, unfinished slots together must fit token_chunk_size, else rwkv_gen_run returns RWKV_ERR_INVALID before any step runs.
 *  - The host runs at most four prompt-carrying steps ahead of the device (the metadata staging ring); nothing else is waited for
 *    between the steps of a run. */
rwkv_status rwkv_gen_arm_prompt(rwkv_engine *e, int32_t slot, const uint32_t *tokens, size_t n_tokens, const rwkv_gen_params *p);
/* prompt tokens of `slot` not yet consumed (0 once it is decoding, or when it is not armed); host-side bookkeeping, no device wait */
rwkv_status rwkv_gen_prompt_left(const rwkv_engine *e, int32_t slot, size_t *left);
rwkv_status rwkv_gen_disarm(rwkv_engine *e, int32_t slot);      /* drop the context (`finish`, run.rs:1007-1020); the state stays as the rule says */
/* Up to n_steps decode steps (run.rs:788-1020, one `infer` + `sample` each) for every armed, unfinished slot.  out_tokens / out_probs:
 * [n_steps][max_batch], step-major, 0xFFFFFFFF / NaN where a slot emitted nothing in that step (out_probs may be NULL; it carries what
 * rwkv_infer_sample's does: the token's probability, or its surprise for Mirostat); pinned or pageable.  n_emitted / finish: [max_batch],
 * tokens the slot emitted IN THIS CALL and RWKV_GEN_* (both may be NULL; RWKV_GEN_HANDBACK only for a slot with stop strings).  With nothing armed: RWKV_OK, nothing emitted.  A launch error is
 * returned by this call, never stale tokens. */
rwkv_status rwkv_gen_run(rwkv_engine *e, int32_t n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish);
/* `tokenizer.decode(&[token])` for every id (run.rs:856): `bytes` is the concatenation of the tokens' bytes in id order, lens[i] the length
 * of id i, or -1 for an id that is not in the vocabulary (ids >= n_tokens are not either): such an id is the reference's decode error, an
 * empty word and a stop (run.rs:858-862).  A token longer than RWKV_GEN_TOKEN_LEN: RWKV_ERR_UNSUPPORTED.  Copied.  May be called again; that
 * disarms nothing, but is refused (RWKV_ERR_INVALID) while any slot has stop strings set. */
rwkv_status rwkv_gen_set_token_bytes(rwkv_engine *e, const uint8_t *bytes, const int32_t *lens, size_t n_tokens);
typedef struct rwkv_gen_stops rwkv_gen_stops;
struct rwkv_gen_stops {
    const uint8_t *const *strs;    /* `GenerateRequest::stop` as bytes (run.rs:905), n <= RWKV_GEN_MAX_STOP_STR strings of <= RWKV_GEN_STOP_LEN bytes */
    const size_t *lens;
    size_t n;
    const uint8_t *tail;           /* `context.buffer` (run.rs:869, 1010) as the caller's own matcher holds it after the tokens it handled itself:  */
    size_t n_tail;                 /*   non-empty after rwkv_gen_arm (whose first_token the caller sampled and matched), normally empty after       */
};                                 /*   rwkv_gen_arm_prompt; n_tail <= RWKV_GEN_STOP_BUF                                                           */
/* The stop strings of an armed, unfinished slot (run.rs:899-932), set between runs; replaces strings and buffer, n = 0 clears them.  Copied.
 * RWKV_ERR_INVALID: the slot is not armed (or has finished), no token table, a NULL array.  RWKV_ERR_UNSUPPORTED: one of the limits above.
 * Re-arming a slot and everything that disarms it clear its strings. */
rwkv_status rwkv_gen_set_stops(rwkv_engine *e, int32_t slot, const rwkv_gen_stops *s);
/* The slot's buffer as it stands (`context.buffer` after `buffer = tail`, run.rs:1010): *len bytes, of which min(*len, cap) are copied to
 * `out` (may be NULL with cap = 0).  Waits for the device.  For a caller that resumes per token after RWKV_GEN_HANDBACK or between runs. */
rwkv_status rwkv_gen_stop_tail(rwkv_engine *e, int32_t slot, uint8_t *out, size_t cap, size_t *len);
/* the draws `first_step .. first_step + n - 1` of (seed, stream): pure host function, no device needed */
rwkv_status rwkv_gen_uniform(uint64_t seed, uint32_t stream, uint32_t first_step, size_t n, float *out);

/* ---- A WATCH: stream tokens out of a running rwkv_gen_run and cancel slots inside it.  The reference sends every token to the client as
 * it is drawn (run.rs:1009, `sender.send(Token::Content(word))`) and ends a request as soon as its client is gone (run.rs:934-935,
 * `context.sender.is_disconnected()` -> `done`); rwkv_gen_run shows nothing until it returns and could drop a request only between runs.
 * With a watch open another thread sees every step as it ends and can reach into the run — without a HIP call, and without the device
 * ever waiting for the host.  With no watch open a step launches what it launched before, from the same cached graphs.
 *   LIFETIME.  At most one watch per engine: a second open is RWKV_ERR_INVALID, and so is ring_steps outside 1 .. RWKV_GEN_WATCH_MAX_STEPS.
 *     open and close run on the infer thread, between runs; the engine's destructor closes an open watch.  open, close and rwkv_engine_destroy
 *     must not run concurrently with read, head or cancel: the caller's duty, as for every handle here.  A watch holds
 *     ring_steps x (8 + 12 max_batch, padded to 16) + 16 + 4 max_batch bytes of pinned host memory, mapped and coherent.
 *   PUBLISHING.  While a watch is open every step of rwkv_gen_run / rwkv_gen_run_topn publishes one RECORD, a step that emits no row
 *     included (a step in which every slot is still inside its prompt).  A record holds, per slot, the step's cell of out_tokens
 *     (0xFFFFFFFF where the slot emitted nothing), its cell of out_probs, and the slot's `finish` after the step (0 for a slot that was
 *     never armed).  Records carry a sequence number that counts from 0 at open and runs on across the engine's internal ring splits and
 *     across runs.  The records of a run are, bit for bit and in order, the rows of out_tokens / out_probs the run executed; rows it did
 *     not execute stay padding and have no record.  Top-n lists are not published: they arrive with rwkv_gen_run_topn as before.
 *     rwkv_gen_run's own outputs stay authoritative and complete.
 *   READING.  rwkv_gen_watch_read copies the records *cursor .. (at most max_steps; tokens / probs / finish are [max_steps][max_batch],
 *     probs and finish may be NULL), sets *n_steps and advances *cursor; a fresh reader starts with *cursor = 0.  It never blocks, makes
 *     no HIP call and takes no lock.  The device never waits for a reader: one that fell more than ring_steps behind gets *lost = the
 *     number of records it skipped and continues at the oldest record still intact.  A record is NEVER returned torn or overwritten
 *     (a sequence lock per record, csrc/gen_watch.h).  One reader per cursor; any number of cursors.  rwkv_gen_watch_head: the number of
 *     records published so far.
 *   CANCELLING.  rwkv_gen_watch_cancel sets the slot's flag; arming the slot (rwkv_gen_arm, rwkv_gen_arm_prompt) and everything that
 *     disarms it (rwkv_gen_disarm, a rwkv_infer / state call on the slot) clear it.  A flag on an unarmed or finished slot does nothing.
 *     With no watch open flags do not exist: cancellation is a facility of the watch.
 *      - A DECODING slot whose flag is seen ends in the first step that sees it: the token it drew in that step is emitted as its last
 *        token, finish = RWKV_GEN_CANCELLED, and the STATE RULE holds unchanged — everything consumed except that last token, the state
 *        the reference caches on `done`.  If the slot finished by itself in that very step its own reason stands.
 *        Its penalties, stop-string buffer (rwkv_gen_stop_tail), DFA state and stack configuration are those of a RUNNING slot at that
 *        point, i.e. BEHIND the last token — not the "buffer as before the last token" of a slot that finished by a stop.
 *      - A slot still INSIDE ITS PROMPT is cancelled by the host when it plans the next step: it is planned no more, emits nothing, its
 *        state has consumed the prompt tokens fed so far, rwkv_gen_prompt_left keeps what was left, and finish = RWKV_GEN_CANCELLED when
 *        the run returns (the records show its finish from the next run on).
 *      - Which step sees a flag set during a run is not deterministic.  Everything returned is a prefix of the uncancelled output, and
 *        no other slot changes by a bit. */
#define RWKV_GEN_CANCELLED 4            /* joins RWKV_GEN_RUNNING / _STOP / _LENGTH / _HANDBACK: the request was cancelled through a watch */
#define RWKV_GEN_WATCH_MAX_STEPS 65536
typedef struct rwkv_gen_watch rwkv_gen_watch;
rwkv_status rwkv_gen_watch_open(rwkv_engine *e, int32_t ring_steps, rwkv_gen_watch **out);   /* infer thread, between runs */
rwkv_status rwkv_gen_watch_close(rwkv_engine *e, rwkv_gen_watch *w);                         /* infer thread, between runs */
rwkv_status rwkv_gen_watch_head(const rwkv_gen_watch *w, uint64_t *seq);                     /* ANY thread */
rwkv_status rwkv_gen_watch_read(rwkv_gen_watch *w, uint64_t *cursor, int32_t max_steps, uint32_t *tokens, float *probs, int32_t *finish,
                                int32_t *n_steps, uint64_t *lost);                           /* ANY thread, one reader per cursor */
rwkv_status rwkv_gen_watch_cancel(rwkv_gen_watch *w, int32_t slot);                          /* ANY thread */

/* ---- `Formatter` (sampler/bnf.rs:34-48; run.rs:676-680 `transform`, 892-897 `update`, 990 halt) for REGULAR constraints: a byte-level DFA.
 * The reference's formatter is kbnf, a context-free engine that lives on the host; this is a second implementation of the same trait for
 * what a finite automaton can say (enumerations, numbers, dates, fixed-field JSON objects), NOT kbnf and no port of it.
 *   - The automaton: trans[n_states][256] (uint16, row-major), accepting[n_states], a start state.  State 0 is DEAD: its row is all zeros
 *     and it accepts nothing.  A state is LIVE when it is not 0.  n_states <= RWKV_DFA_MAX_STATES, DEAD included.
 *   - ALLOWED (`transform`, bnf.rs:35-38): in state q token v is allowed iff v < n_tokens of the token table, its entry is known and
 *     NON-EMPTY, and walking its bytes from q ends in a live state.  Token 0 (the end-of-sequence id, run.rs:855, whatever a table says
 *     of it; the World vocabulary has no entry for it), empty tokens (bnf.rs:18) and unknown ids are never allowed, so a constrained request ends by halt, stop token, stop string or max_tokens, never by a sampled EOS.  A masked logit is -inf before
 *     the softmax; penalties and bias add to -inf and leave it -inf, so their order against the mask is immaterial (run.rs:676-683).
 *     DEVIATION from the reference, on purpose: bnf.rs:36 masks only output[..vocab_size] and leaves the ids between the tokenizer's size
 *     and num_vocab untouched; here they are masked, because they decode to the reference's error-and-stop (run.rs:858-862).
 *   - ADVANCE (`update`, bnf.rs:40-48): after a draw the state moves over the drawn token's bytes.  A drawn token that is not allowed
 *     leaves the state where it was and does not halt (kbnf rejects it and goes on, bnf.rs:44).
 *   - HALT, per slot: RWKV_DFA_HALT_FINAL — the new state accepts and no byte leads from it to a live state; RWKV_DFA_HALT_ACCEPT — the
 *     new state accepts.  Halt is or-ed into the token-stop predicate (`halt || stop_matched || stop_token`, run.rs:990: FinishReason::Stop,
 *     before max_tokens).  The halting token is emitted as the slot's last token and the STATE RULE above holds unchanged.
 * Handles are immutable and thread-safe, like tokenizer handles; every rwkv_dfa_* function is a pure host function, no device needed. */
#define RWKV_DFA_MAX_STATES 4096
enum { RWKV_DFA_HALT_FINAL = 0, RWKV_DFA_HALT_ACCEPT = 1 };
typedef struct rwkv_dfa rwkv_dfa;
/* any compiler's output (json2kbnf.py-style helpers may target it).  RWKV_ERR_INVALID: state 0 is not dead, a target >= n_states, start
 * outside [1, n_states), n_states < 2, a NULL array.  RWKV_ERR_UNSUPPORTED: n_states > RWKV_DFA_MAX_STATES.  Nothing is trimmed or
 * renumbered; accepting[] is read as zero / non-zero.  Copied. */
rwkv_status rwkv_dfa_from_table(const uint16_t *trans, const uint8_t *accepting, int32_t n_states, int32_t start, rwkv_dfa **out);
/* A small ANCHORED regex dialect (the whole output must match), `GenerateRequest::bnf_schema`'s regular cousin (docs/doc-guide/features.md "BNF"):
 *   literals   UTF-8 text (a multi-byte character is one atom)
 *   escapes    \n \r \t \\ \" \/ \xHH, an escaped metacharacter ( . [ ] ( ) { } | * + ? ^ $ - ), \d = [0-9], \w = [A-Za-z0-9_], \s = [ \t\r\n]
 *   classes    [...] of ASCII members and ranges; [^...] = any WELL-FORMED UTF-8 character (Unicode table 3-7, the rule of the stop-string
 *              buffer) that is not in the ASCII set; . = [^\n]
 *   structure  ( ) | * + ? {m} {m,} {m,n} with counts <= 255; a repeat of a repeat needs a group
 * Thompson NFA -> subset construction -> trim (a state that cannot reach an accepting state becomes DEAD) -> minimise -> canonical
 * numbering (breadth-first from the start state, bytes ascending, start = 1): a language has exactly one table, whatever its spelling.
 * RWKV_ERR_INVALID: a malformed pattern, with the byte offset in rwkv_last_error.  RWKV_ERR_UNSUPPORTED: the pattern matches nothing, or
 * needs too many states (RWKV_DFA_MAX_STATES after minimisation, or the compiler's own working limits before it). */
rwkv_status rwkv_dfa_compile(const uint8_t *pattern, size_t len, rwkv_dfa **out);
void rwkv_dfa_free(rwkv_dfa *d);
int32_t rwkv_dfa_num_states(const rwkv_dfa *d);
int32_t rwkv_dfa_start(const rwkv_dfa *d);
/* reads the table back: trans[num_states * 256], accepting[num_states] (either may be NULL) */
rwkv_status rwkv_dfa_table(const rwkv_dfa *d, uint16_t *trans, uint8_t *accepting);
/* the state `n` bytes behind `state` (0 once the walk died) */
rwkv_status rwkv_dfa_walk(const rwkv_dfa *d, int32_t state, const uint8_t *bytes, size_t n, int32_t *next);
/* `transform` on the host: the num_vocab-byte mask rwkv_sample_params.allow takes, by the ALLOWED rule above; `bytes` / `lens` / n_tokens as
 * in rwkv_gen_set_token_bytes.  The per-token path gets the same formatter without a device, and a caller can hand a request over between
 * the two paths in either direction (rwkv_gen_constraint_state). */
rwkv_status rwkv_dfa_allow(const rwkv_dfa *d, int32_t state, const uint8_t *bytes, const int32_t *lens, size_t n_tokens, uint8_t *allow,
                           size_t num_vocab);
/* The LIVENESS rule of rwkv_gen_set_constraint as a pure host function, over a token table given as to rwkv_gen_set_token_bytes (note
 * the order: lens first): RWKV_OK, or RWKV_ERR_UNSUPPORTED when a state the slot can come to rest in has no single-byte token that leads to
 * a live state.  O(states x 256). */
rwkv_status rwkv_dfa_check_live(const rwkv_dfa *d, int32_t state, int32_t halt_mode, const int32_t *lens, const uint8_t *bytes, size_t n_tokens);
/* The constraint of an armed, unfinished slot, set between runs like rwkv_gen_set_stops; the table is copied to the device, `dfa` may be
 * freed on return.  `state`: the start state after rwkv_gen_arm_prompt; after rwkv_gen_arm the state behind first_token, which the
 * caller sampled and advanced itself.  dfa == NULL clears the constraint; re-arming a slot and everything that disarms it clear it too.
 * From then on every step masks the slot's row on the device (the tokens that are not ALLOWED become -inf between the penalties and the
 * sampling kernel), advances the state behind the drawn token and tests HALT; steps in which no slot has a constraint launch what they
 * launched before.
 * RWKV_ERR_INVALID: the slot is not armed or has finished, no token table (rwkv_gen_set_token_bytes), state 0 or out of range, a bad
 * halt_mode.  RWKV_ERR_UNSUPPORTED: LIVENESS — every live state reachable from `state` in which the slot can come to rest (one that does
 * not halt) must have a SINGLE-BYTE token of the table that leads to a live state, which is what guarantees that a row is never all -inf
 * (the World vocabulary holds all 256 single-byte tokens).  rwkv_gen_set_token_bytes is refused while any slot has a constraint.
 * Also RWKV_ERR_INVALID: the slot has a stack constraint (rwkv_gen_set_pda below) — a slot holds one kind or the other. */
rwkv_status rwkv_gen_set_constraint(rwkv_engine *e, int32_t slot, const rwkv_dfa *dfa, int32_t state, int32_t halt_mode);
/* The state behind every token the slot has emitted, the last one included (0 for a slot without a constraint).  Waits for the device. */
rwkv_status rwkv_gen_constraint_state(rwkv_engine *e, int32_t slot, int32_t *state);

/* ---- `Formatter` for NESTED constraints: a byte automaton whose `{` / `[` transitions push a return state and whose `}` / `]` transitions
 * pop one.  A third implementation of the trait, beside kbnf on the host and the DFA above; NOT kbnf and no port of it.  It exists because
 * nesting has no finite automaton of useful size (the object-or-array context of every level doubles the states of a DFA), and "answer in
 * JSON" is the request an OpenAI-style server gets most.  General context-free grammars keep the per-token path.
 *   - TABLES: states 0 .. n_states - 1, n_states <= RWKV_PDA_MAX_STATES.  State 0 is DEAD: both of its rows are zero and it accepts
 *     nothing.  Two uint16 planes [n_states][256] (row-major), `next` and `act`, accepting[n_states], a start state, and max_depth in
 *     1 .. RWKV_PDA_MAX_DEPTH.
 *   - TRANSITIONS, for state q and byte b:  act == 0 is PLAIN: go to next; next == 0 is dead.  act == RWKV_PDA_POP is a POP: the next state
 *     is the popped entry; an empty stack is dead; `next` is ignored.  Any other act is a PUSH: act must be a live state id and next must be
 *     non-zero; act is pushed as the return state and the automaton goes to next; a stack that already holds max_depth entries is dead.
 *   - CONFIGURATION: (state, stack of uint16, bottom first).  LIVE: state != 0.  ACCEPTS: accepting[state] and an empty stack.  END, a
 *     per-state flag computed on the host: no plain or push entry with a live target (pops do not count: the stack is empty where it matters).
 *   - ALLOWED follows the DFA rule — token v is in the table, known, non-empty and not id 0, and walking its bytes ends LIVE — with one
 *     addition, THE SPAN RULE: while a token is walked, let `low` be the smallest depth reached so far; a push that would make
 *     depth - low > RWKV_PDA_TOKEN_SPAN makes the token not allowed.  Host (rwkv_pda_allow) and device apply the same rule, so it is
 *     part of the language, not an implementation limit.  (rwkv_pda_walk walks BYTES and knows no tokens: no span rule there.)
 *   - ADVANCE: a drawn token that is not allowed leaves the configuration where it was and does not halt.
 *   - HALT: RWKV_PDA_HALT_FINAL — the new configuration ACCEPTS and its state is END; RWKV_PDA_HALT_ACCEPT — it ACCEPTS.  Or-ed into the
 *     stop predicate exactly where the DFA's halt is; the STATE RULE of rwkv_gen_run is unchanged.
 *   - LIVENESS, checked when the constraint is set (and by rwkv_pda_check_live), else RWKV_ERR_UNSUPPORTED.  Conservative and static,
 *     O(states x 256): from the configuration, every state any sequence of transitions could enter is collected (plain and push targets,
 *     and every return state a collected state pushes), each with one bit: whether it is only ever entered WITH AN EMPTY STACK.  Every
 *     collected state must have a single-byte token of the table with a PLAIN live transition — plain works at every depth, max_depth
 *     included, where every push is dead.  A state only ever entered with an empty stack may use a PUSH instead (it cannot fail there:
 *     max_depth >= 1).  The only exempt state is one that is only ever entered ACCEPTING-and-END (accepting, END, empty stack: it halts
 *     in both modes), and never the configuration's own state.  This guarantees that no row is all -inf at any depth.  The JSON automaton
 *     below satisfies it over the World vocabulary, which holds all 256 single-byte tokens.
 * Handles are immutable and thread-safe; every rwkv_pda_* function is a pure host function, no device needed. */
#define RWKV_PDA_MAX_STATES 4096
#define RWKV_PDA_MAX_DEPTH 64
#define RWKV_PDA_TOKEN_SPAN 8
#define RWKV_PDA_POP 65535                    /* 0xFFFF in `act` */
enum { RWKV_PDA_HALT_FINAL = 0, RWKV_PDA_HALT_ACCEPT = 1 };
enum { RWKV_PDA_JSON_OBJECT = 1, RWKV_PDA_JSON_COMPACT = 2 };     /* flags of rwkv_pda_json */
typedef struct rwkv_pda rwkv_pda;
/* any compiler's output (a schema-to-automaton compiler may target it).  RWKV_ERR_INVALID: the rwkv_dfa_from_table conditions (state 0
 * not dead in either plane, a target >= n_states, start outside [1, n_states), n_states < 2, a NULL array), an act that is neither 0,
 * RWKV_PDA_POP nor a live state id, a push with next == 0, max_depth outside 1 .. RWKV_PDA_MAX_DEPTH.  RWKV_ERR_UNSUPPORTED:
 * n_states > RWKV_PDA_MAX_STATES.  Nothing is trimmed or renumbered.  Copied. */
rwkv_status rwkv_pda_from_table(const uint16_t *next, const uint16_t *act, const uint8_t *accepting, int32_t n_states, int32_t start,
                                int32_t max_depth, rwkv_pda **out);
/* RFC 8259 over bytes.  Strings hold well-formed UTF-8 only (Unicode table 3-7, the rule rwkv_dfa_compile uses for [^...]) and no byte
 * below 0x20; escapes are \" \\ \/ \b \f \n \r \t \uXXXX.  Numbers are -?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?; a number has no terminator,
 * so the states it may end in take over the row of the state behind a value.  Nesting deeper than max_depth is refused (dead).
 *   RWKV_PDA_JSON_OBJECT   the top-level value must be an object or an array (without it `1` accepts behind its first digit, which
 *                          together with RWKV_PDA_HALT_ACCEPT is rarely wanted)
 *   RWKV_PDA_JSON_COMPACT  no whitespace outside strings (the usual failure of JSON mode is a run of newlines until max_tokens)
 * The numbering is canonical — breadth-first from the start state (= 1), bytes ascending, a push's target before its return state — one
 * table per `flags`, independent of max_depth.  RWKV_ERR_INVALID: an unknown flag, max_depth out of range. */
rwkv_status rwkv_pda_json(uint32_t flags, int32_t max_depth, rwkv_pda **out);
void rwkv_pda_free(rwkv_pda *p);
int32_t rwkv_pda_num_states(const rwkv_pda *p);
int32_t rwkv_pda_start(const rwkv_pda *p);
int32_t rwkv_pda_max_depth(const rwkv_pda *p);
/* reads the table back: next[num_states * 256], act[num_states * 256], accepting[num_states] (each may be NULL) */
rwkv_status rwkv_pda_table(const rwkv_pda *p, uint16_t *next, uint16_t *act, uint8_t *accepting);
/* the configuration `n` bytes behind (state, stack[0 .. depth)): *state_out is 0 once the walk died (the stack is then what it was at the
 * byte that killed it).  stack_out has room for max_depth entries and may be `stack` itself.  RWKV_ERR_INVALID: a state, depth or stack
 * entry out of range. */
rwkv_status rwkv_pda_walk(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const uint8_t *bytes, size_t n,
                          int32_t *state_out, uint16_t *stack_out, int32_t *depth_out);
/* `transform` on the host: the num_vocab-byte mask rwkv_sample_params.allow takes, by the ALLOWED rule above (the span rule included), so
 * the per-token path gets the same formatter and a request can be handed over in either direction (rwkv_gen_pda_config). */
rwkv_status rwkv_pda_allow(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const uint8_t *bytes, const int32_t *lens,
                           size_t n_tokens, uint8_t *allow, size_t num_vocab);
/* the LIVENESS rule as a pure host function, over a token table given as to rwkv_gen_set_token_bytes (note the order: lens first) */
rwkv_status rwkv_pda_check_live(const rwkv_pda *p, int32_t state, const uint16_t *stack, int32_t depth, const int32_t *lens, const uint8_t *bytes,
                                size_t n_tokens);
/* The stack constraint of an armed, unfinished slot, set between runs like rwkv_gen_set_constraint; the table is copied to the device,
 * `pda` may be freed on return.  Any configuration is accepted: the start state with an empty stack after rwkv_gen_arm_prompt, or the
 * caller's own after rwkv_gen_arm or a hand-over.  pda == NULL clears the constraint; re-arming a slot and everything that disarms it
 * clear it too.  From then on every step masks the slot's row on the device, commits the drawn token to the slot's configuration and tests
 * HALT; a step in which no slot has a stack constraint launches what it launched before.
 * A slot holds a DFA or a stack constraint: setting one while the other is set is RWKV_ERR_INVALID.  Also RWKV_ERR_INVALID: the slot is not
 * armed or has finished, no token table, state 0 or out of range, depth outside 0 .. max_depth, a stack entry that is no live state, a bad
 * halt_mode.  RWKV_ERR_UNSUPPORTED: LIVENESS.  rwkv_gen_set_token_bytes is refused while any slot has a constraint of either kind. */
rwkv_status rwkv_gen_set_pda(rwkv_engine *e, int32_t slot, const rwkv_pda *pda, int32_t state, const uint16_t *stack, int32_t depth,
                             int32_t halt_mode);
/* The configuration behind every token the slot has emitted, the last one included: *state (0 for a slot without a stack constraint),
 * *depth, and min(*depth, cap) entries of the stack, bottom first (stack may be NULL with cap = 0).  Waits for the device. */
rwkv_status rwkv_gen_pda_config(rwkv_engine *e, int32_t slot, int32_t *state, uint16_t *stack, size_t cap, int32_t *depth);

/* ---- top-n lists in resident generation: what else the model considered, per emitted token, without the row leaving the device.
 * The distribution is the RAW MODEL ROW — what the head wrote, before penalties, bias, temperature and any constraint mask — the definition
 * rwkv_infer_score uses, and the one a caller cannot reconstruct from anything else the run returns.
 * rwkv_gen_set_topn: an armed, unfinished slot lists its n (0 .. RWKV_TOPN_MAX; 0 = off) most likely tokens with every token it emits from now
 * on; re-arming the slot resets n to 0.  The first call allocates max_batch * num_vocab * 4 bytes of device memory for the raw rows.
 * rwkv_gen_run_topn is rwkv_gen_run — the first six arguments behave exactly as there — with three more outputs, step-major like out_tokens:
 *   out_tok_logp [n_steps][max_batch]         the raw ln-probability of the emitted token: rwkv_score_rows' value for the raw row and that token,
 *                                             bit for bit (and the list's entry, when the token is listed)
 *   out_top_ids  [n_steps][max_batch][n_top]  the slot's list (see "top-n lists on the device" above), its own n places; the places up to the
 *   out_top_logp                              caller's stride n_top hold (RWKV_TOPN_NONE, -inf)
 * Where a slot emitted nothing in a step: (RWKV_TOPN_NONE, NaN) and NaN in out_tok_logp; a slot with n == 0 has NaN in out_tok_logp too.
 * n_top (1 .. RWKV_TOPN_MAX) must be >= every armed, unfinished slot's n, else RWKV_ERR_INVALID before the first step.
 * INVARIANT: listing changes no token, probability, finish reason, stop tail, constraint state or state of any slot — the extra launch only
 * reads the logits block — and a step in which no slot lists is the step rwkv_gen_run ran before, launch for launch.  rwkv_gen_run stays
 * callable on listing slots and returns what it returned before. */
rwkv_status rwkv_gen_set_topn(rwkv_engine *e, int32_t slot, int32_t n);
rwkv_status rwkv_gen_run_topn(rwkv_engine *e, int32_t n_steps, uint32_t *out_tokens, float *out_probs, int32_t *n_emitted, int32_t *finish,
                              int32_t n_top, float *out_tok_logp, uint32_t *out_top_ids, float *out_top_logp);

/* ---- captures and items: resident generation fills and uses the prefix cache.  The reference caches CachedItem(state, output) pairs
 * (run.rs:201-223) at two points of `process`: when the prompt's last row arrives (run.rs:834-845) and when a request stops
 * (run.rs:995-1001); a request whose whole prompt is cached samples straight from the cached row, `(0, Some(output)) => output`
 * (run.rs:809-810).  An ITEM is such a pair on the device: a state and the RAW head row — before penalties, bias, temperature and masks,
 * the definition rwkv_gen_set_topn uses.  It is immutable, owns its memory, and outlives the slot and the engine that made it.
 * The threading contract is that of rwkv_infer.
 *   rwkv_gen_set_capture: what an armed, unfinished slot keeps, set between runs like rwkv_gen_set_stops.  `what` is a set of
 *     RWKV_GEN_CAPTURE_* bits; a bit that is clear drops that item if nobody took it, so 0 clears everything; an unknown bit is RWKV_ERR_INVALID, and so is PROMPT on a slot with
 *     rwkv_gen_prompt_left == 0.  Re-arming the slot and everything that disarms it clear the setting and drop any item not taken.  The
 *     call allocates what the capture needs (one state and one row per bit); nothing is allocated inside a run.
 *   The PROMPT item: the slot's state after it has consumed exactly its prompt, on top of the state the prompt was armed on, and the raw
 *     row of the prompt's last token.  Both are taken in the step that exhausts the prompt; the item can be taken as soon as that run has
 *     returned, while the slot goes on decoding.
 *   The FINISH item: complete when the slot finishes, for any reason but a cancel inside its prompt.  The state the STATE RULE prescribes
 *     (everything consumed except the last emitted token) and the raw row of the step the slot finished in — the row its last token was
 *     drawn from.  A slot that finishes on its first draw has FINISH == PROMPT, bit for bit.  Taken while the slot stays armed and finished.
 *   rwkv_gen_take_item: `which` is exactly one bit.  RWKV_ERR_INVALID when the item was not asked for, is not complete yet (the prompt is
 *     not exhausted, the slot still runs, it was cancelled inside its prompt) or was already taken.  Ownership passes to the caller
 *     (rwkv_gen_item_free; NULL is fine).
 *   INVARIANT: capturing changes no token, probability, finish reason, stop tail, constraint state, top-n list, watch record or state of
 *     any slot — the extra launch reads the logits block and the state and writes item memory only — and a step in which no slot captures
 *     launches what it launched before, from the same captured graphs.
 *   rwkv_gen_item_state: the item's state, borrowed, for rwkv_state_write (a PARTIAL prefix hit continues with rwkv_gen_arm_prompt).  It is
 *     a const rwkv_dstate * that lives as long as the item and must not go to rwkv_dstate_free; NULL for a NULL item.
 *   rwkv_gen_item_back / _from_host: `state` in the slab layout of rwkv_state_back (rwkv_state_len floats), `row` num_vocab floats; either
 *     destination of _back may be NULL.  The round trip is bit-exact.  An item is accepted by any engine whose device, model version
 *     and dimensions match its maker's, else RWKV_ERR_INVALID.
 *   rwkv_gen_arm_item: rwkv_gen_arm_prompt for a prompt that is wholly cached.  The slot's state becomes the item's; `p` is read as
 *     rwkv_gen_arm_prompt reads it (first_token ignored, the penalty arrays are the map after `init(prompt)`).  In its FIRST STEP the slot
 *     consumes nothing: its first token is drawn on the device from the item's row with draw counter 0 of (seed, stream), by the
 *     arithmetic of any draw; penalty and Mirostat updates, the stop, constraint and max_tokens tests follow as after any draw.  From the
 *     next step on it is a decoding slot.  It counts as one row towards token_chunk_size; a step whose only participants are such slots
 *     runs no forward pass.  The refusals of rwkv_gen_arm apply, every one as RWKV_ERR_INVALID, and leave the slot as it was.  The item is only read and is free again when the call returns; it may
 *     arm any number of slots. */
#define RWKV_GEN_CAPTURE_PROMPT 1u
#define RWKV_GEN_CAPTURE_FINISH 2u
typedef struct rwkv_gen_item rwkv_gen_item;     /* CachedItem run.rs:201-223: a device-resident (state, raw logits row) pair; immutable */
rwkv_status rwkv_gen_set_capture(rwkv_engine *e, int32_t slot, uint32_t what);
rwkv_status rwkv_gen_take_item(rwkv_engine *e, int32_t slot, uint32_t which, rwkv_gen_item **out);
void rwkv_gen_item_free(rwkv_gen_item *it);
const void *rwkv_gen_item_state(const rwkv_gen_item *it);   /* a const rwkv_dstate *, owned by the item: hand it to rwkv_state_write */
rwkv_status rwkv_gen_item_back(rwkv_engine *e, const rwkv_gen_item *it, float *state_dst, float *row_dst);
rwkv_status rwkv_gen_item_from_host(rwkv_engine *e, const float *state, const float *row, rwkv_gen_item **out);
rwkv_status rwkv_gen_arm_item(rwkv_engine *e, int32_t slot, const rwkv_gen_item *it, const rwkv_gen_params *p);

/* ---- `Tokenizer` lib.rs:375; run.rs:157-168,856; sampler/bnf.rs:14-27 ---------------------- */
typedef struct rwkv_tokenizer rwkv_tokenizer;
rwkv_status rwkv_tokenizer_create(const char *vocab_json, size_t len, rwkv_tokenizer **out);
void rwkv_tokenizer_destroy(rwkv_tokenizer *t);
/* returns number of tokens (may exceed cap: call again with a larger buffer), <0 on error */
int64_t rwkv_tokenizer_encode(const rwkv_tokenizer *t, const uint8_t *text, size_t len, uint32_t *out, size_t cap);
/* returns number of bytes (may exceed cap), <0 on error (unknown token id) */
int64_t rwkv_tokenizer_decode(const rwkv_tokenizer *t, const uint32_t *tokens, size_t n, uint8_t *out, size_t cap);
int64_t rwkv_tokenizer_token_bytes(const rwkv_tokenizer *t, uint32_t token, uint8_t *out, size_t cap);
int64_t rwkv_tokenizer_vocab_size(const rwkv_tokenizer *t);   /* highest id + 1 */

/* ---- measurement hooks (bench.py; not part of the reference surface) -----------------------
 * rwkv_profile_infer runs the same step as rwkv_infer but brackets every kernel launch with
 * hipEvents on the engine's compute stream and accumulates per-kernel-family milliseconds.
 * Families: see rwkv_profile_family_name.  `ms` has RWKV_PROFILE_FAMILIES entries. */
#define RWKV_PROFILE_FAMILIES 8
const char *rwkv_profile_family_name(int32_t family);
rwkv_status rwkv_profile_infer(rwkv_engine *e, const rwkv_slot_input *in, rwkv_slot_output *out,
                               float *ms, int32_t *launches);
/* device-resident greedy decode (f-1 front-end, arg-max only): runs `n_steps` decode steps for the
 * first `n_slots` slots, feeding each slot's arg-max token back on the device; only token ids
 * cross PCIe.  first_tokens[n_slots] in, out_tokens[n_steps*n_slots] (step-major) out.
 * Returns milliseconds of device time for the timed region in *elapsed_ms (hipEvents). */
rwkv_status rwkv_decode_greedy(rwkv_engine *e, int32_t n_slots, const uint32_t *first_tokens,
                               int32_t n_steps, uint32_t *out_tokens, float *elapsed_ms);

/* kernel microbench: one [rows x K] GEMM problem in weight format `fmt` (0 fp16, 1 int8, 2 nf4, 3 sf4) against T
 * activation rows; `nmat` distinct weight copies are rotated so re-reads miss the Infinity Cache.
 * ksw = 0 lets the planner choose the in-block K split.  Returns microseconds per launch. */
rwkv_status rwkv_bench_gemm(int32_t rows, int32_t K, int32_t fmt, int32_t T, int32_t hilo, int32_t ksw,
                            int32_t nmat, int32_t iters, float *us_per_launch, float *lds_kib);

#ifdef __cplusplus
}
#endif
#endif /* RWKV_ABI_H */
