//! Safe wrapper over `librwkv_hip.so` for ai00-core.  NOT compiled in the image this repository is built in (no rustc there):
//! written against `include/rwkv_abi.h`; `integration/check.sh` type-checks it on a machine with Rust.
//!
//! Layout: the plain wrapper (`Engine`, `Tokenizer`, `Error`) and, in `compat`, the same calls under the names and shapes
//! `crates/ai00-core/src/{lib,run}.rs` import from `web_rwkv` (lib.rs:24-35, run.rs:22-31), so that `ai00-core.patch` is an
//! import change plus the five call sites that construct things.
//!
//! Threading contract (run.rs:1072-1190): per engine one thread calls `infer` + the state functions (the `infer` task) and one
//! calls `softmax` (the `softmax` task).  `Engine` is `Send + Sync` on that contract; the library serialises nothing for you.
use rwkv_hip_sys as sys;
use std::{ffi::{CStr, CString}, os::raw::c_void, ptr, sync::Arc};

#[derive(Debug, thiserror::Error)]
#[error("librwkv_hip error {code}: {message}")]
pub struct Error { pub code: i32, pub message: String }
pub type Result<T> = std::result::Result<T, Error>;

fn check(rc: i32) -> Result<()> {
    if rc == 0 { return Ok(()); }
    let message = unsafe { CStr::from_ptr(sys::rwkv_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

pub use sys::rwkv_model_info as RawInfo;

/// `list_adapters` (lib.rs:339-349)
pub fn list_adapters() -> Vec<String> {
    (0..unsafe { sys::rwkv_device_count() }).filter_map(|i| {
        let mut buf = vec![0i8; 256];
        (unsafe { sys::rwkv_device_name(i, buf.as_mut_ptr() as *mut _, buf.len()) } == 0)
            .then(|| unsafe { CStr::from_ptr(buf.as_ptr() as *const _) }.to_string_lossy().into_owned())
    }).collect()
}

/// `Loader::info(&SafeTensors)` (lib.rs:587).  `bytes`: the mmap of a `.st` file or of a prefab image (sniffed by content).
pub fn model_info(bytes: &[u8]) -> Result<RawInfo> {
    let mut out = RawInfo::default();
    check(unsafe { sys::rwkv_model_info_from_st(bytes.as_ptr(), bytes.len(), &mut out) })?;
    Ok(out)
}

#[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum QuantType { None = 0, Int8 = 1, NF4 = 2, SF4 = 3 }
/// `reload::Precision` (reload.rs:89-94).  `Fp16` holds 1e-3 on logits / state at 32 layers since ABI 7 (the launches that carry a model's
/// f16 operand rounding read hi + lo operands); `Fp16Raw` is the library's all-f16 extension (fastest, not tolerance-holding at depth).
#[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum Precision { Fp16 = 0, Fp32 = 1, Fp16Raw = 2 }
#[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum Adapter { Auto, Economical, Manual(usize) }
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)] pub enum OutputOption { #[default] Last = 0, Full = 1, None = 2 }

pub struct LoadDesc<'a> {
    pub adapter: Adapter, pub quant_layers: usize, pub quant_type: QuantType, pub precision: Precision,
    pub max_batch: usize, pub token_chunk_size: usize, pub model: &'a [u8], pub lora: Vec<(&'a [u8], f32)>,
}

/// = Context + Model + vN::Bundle + TokioRuntime<Rnn> + State of the reference (lib.rs:484-516)
#[derive(Debug)]
pub struct Engine { raw: *mut sys::rwkv_engine, pub info: RawInfo, pub max_batch: usize, pub token_chunk_size: usize }
unsafe impl Send for Engine {}
unsafe impl Sync for Engine {}
impl Drop for Engine { fn drop(&mut self) { unsafe { sys::rwkv_engine_destroy(self.raw) } } }

/// device-resident state snapshot (`TensorGpu<f32, ReadWrite>` of run.rs:351-355); clone = share the handle
#[derive(Debug)]
pub struct DeviceState(*mut sys::rwkv_dstate);
unsafe impl Send for DeviceState {}
unsafe impl Sync for DeviceState {}
impl Drop for DeviceState { fn drop(&mut self) { unsafe { sys::rwkv_dstate_free(self.0) } } }

/// Which of the two cache fill points of `process` a slot keeps (rwkv_gen_set_capture): the prompt's end (run.rs:834-845), the stop
/// (run.rs:995-1001).  `gen_set_capture` takes a sum of them, `gen_take_item` exactly one.
#[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum GenCapture { Prompt = 1, Finish = 2 }
/// `CachedItem` (run.rs:201-223) on the device: a state and the RAW head row it was followed by (rwkv_gen_item).  Immutable; it outlives
/// the slot and the engine that made it; clone the `Arc` to share it, as the reference shares its `TensorGpu`s.
#[derive(Debug)]
pub struct GenItem(*mut sys::rwkv_gen_item);
unsafe impl Send for GenItem {}
unsafe impl Sync for GenItem {}
impl Drop for GenItem { fn drop(&mut self) { unsafe { sys::rwkv_gen_item_free(self.0) } } }

/// pinned host block for the logits of one `infer` call (rwkv_host_alloc): rows land here in one device-to-host copy
#[derive(Debug)]
pub struct PinnedLogits { ptr: *mut f32, floats: usize, in_flight: usize }
unsafe impl Send for PinnedLogits {}
impl PinnedLogits {
    pub fn new(floats: usize) -> Result<Self> {
        let mut p: *mut c_void = ptr::null_mut();
        check(unsafe { sys::rwkv_host_alloc(floats * 4, &mut p) })?;
        Ok(Self { ptr: p as *mut f32, floats, in_flight: 0 })
    }
    /// Panics while a read-back into the block is in flight: only reachable when a `PendingRows` guard was leaked (`std::mem::forget`) — every
    /// other path holds the block's `&mut` borrow until the copy stream has been waited for.
    pub fn as_slice(&self) -> &[f32] {
        assert!(self.in_flight == 0, "PinnedLogits read while an asynchronous read-back is in flight (a PendingRows guard was leaked)");
        unsafe { std::slice::from_raw_parts(self.ptr, self.floats) }
    }
}
impl Drop for PinnedLogits {
    /// A block with a read-back still accounted in flight (leaked guard) is LEAKED, not freed: the DMA may still be writing it.
    fn drop(&mut self) { if self.in_flight == 0 { unsafe { sys::rwkv_host_free(self.ptr as *mut c_void) } } }
}

/// one slot of an `infer` call: `tokens` is drained by what the call consumed (RnnInputBatch, run.rs:1128)
#[derive(Default, Clone, Debug)]
pub struct SlotInput { pub tokens: Vec<u32>, pub option: OutputOption }

/// what `infer_topn` hands back per slot: `rows` lists of `n` places, `ids[r * n + i]` / `logp[r * n + i]` the i-th most likely token of
/// row r and its ln-probability (`sys::RWKV_TOPN_NONE` where the place holds no entry); `tok_logp[r]` the realised token's ln-probability
/// when the slot had targets (empty otherwise)
#[derive(Default, Clone, Debug)]
pub struct TopLists { pub n: usize, pub rows: usize, pub ids: Vec<u32>, pub logp: Vec<f32>, pub tok_logp: Vec<f32> }

impl Engine {
    pub fn load(d: &LoadDesc) -> Result<Self> {
        let lora: Vec<_> = d.lora.iter().map(|(b, a)| sys::rwkv_lora_desc { st_bytes: b.as_ptr(), st_len: b.len(), alpha: *a }).collect();
        let desc = sys::rwkv_load_desc {
            adapter: match d.adapter { Adapter::Auto => sys::RWKV_ADAPTER_AUTO, Adapter::Economical => sys::RWKV_ADAPTER_ECONOMICAL, Adapter::Manual(n) => n as i32 },
            quant_layers: d.quant_layers as i32, quant_type: d.quant_type as i32, precision: d.precision as i32,
            max_batch: d.max_batch as i32, token_chunk_size: d.token_chunk_size as i32,
            st_bytes: d.model.as_ptr(), st_len: d.model.len(),
            lora: if lora.is_empty() { ptr::null() } else { lora.as_ptr() }, n_lora: lora.len(),
        };
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_engine_create(&desc, &mut raw) })?;
        let mut info = RawInfo::default();
        check(unsafe { sys::rwkv_engine_info(raw, &mut info) })?;
        let (max_batch, token_chunk_size) = unsafe { (sys::rwkv_engine_max_batch(raw) as usize, sys::rwkv_engine_token_chunk_size(raw) as usize) };
        Ok(Self { raw, info, max_batch, token_chunk_size })
    }
    pub fn save_prefab(&self, path: &str) -> Result<()> {
        let c = CString::new(path).map_err(|_| Error { code: sys::RWKV_ERR_INVALID, message: "path contains NUL".into() })?;
        check(unsafe { sys::rwkv_engine_save_prefab(self.raw, c.as_ptr()) })
    }
    /// Rows each slot can emit in the NEXT call, computed the way the engine computes them: `rwkv_plan_chunk` is the engine's own
    /// split of the `token_chunk_size` budget over the slots (the call consumes at most `token_chunk_size` tokens IN TOTAL, so two
    /// `Full` slots of 100 tokens at chunk 128 emit 128 rows together, not 200); a `Full` slot emits one row per consumed token, a
    /// `Last` slot one row when the call exhausts its tokens, a `None` slot nothing.  The sum is <= token_chunk_size + max_batch.
    pub fn plan_rows(&self, input: &[SlotInput]) -> Result<Vec<usize>> {
        // `rwkv_plan_chunk` reads `max_batch` entries: a shorter slice would be an out-of-bounds read behind a safe signature
        if input.len() != self.max_batch {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("plan_rows: {} slot inputs for max_batch {}", input.len(), self.max_batch) });
        }
        let pending: Vec<usize> = input.iter().map(|s| s.tokens.len()).collect();
        let mut take = vec![0i32; input.len()];
        check(unsafe { sys::rwkv_plan_chunk(self.max_batch as i32, self.token_chunk_size as i32, pending.as_ptr(), take.as_mut_ptr()) })?;
        Ok(input.iter().zip(&take).map(|(s, &t)| match s.option {
            OutputOption::None => 0,
            OutputOption::Last => usize::from(t > 0 && t as usize == s.tokens.len()),
            OutputOption::Full => t.max(0) as usize }).collect())
    }
    pub fn rows_needed(&self, input: &[SlotInput]) -> Result<usize> { Ok(self.plan_rows(input)?.iter().sum()) }
    /// `runtime.infer(input)` (run.rs:1143): ONE step over <= token_chunk_size tokens.  Consumed tokens are drained from `input`;
    /// returns, per slot, the rows it emitted as `(offset_in_floats, n_rows)` into `logits` (`(0, 0)` for a slot without rows).
    /// Never panics on a caller mistake: a wrong slot count or a block that is too small comes back as `Err` (the infer task treats
    /// it like any other runtime error, run.rs:1143 `?`) instead of taking the server down.
    pub fn infer(&self, input: &mut [SlotInput], logits: &mut PinnedLogits) -> Result<Vec<(usize, usize)>> {
        if input.len() != self.max_batch {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("infer: {} slot inputs for max_batch {}", input.len(), self.max_batch) });
        }
        let v = self.info.num_vocab as usize;
        let rows = self.plan_rows(input)?;
        let total: usize = rows.iter().sum();
        if total * v > logits.floats {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("infer: logits block holds {} rows, the step emits {}", logits.floats / v, total) });
        }
        let inp: Vec<_> = input.iter().map(|s| sys::rwkv_slot_input {
            tokens: if s.tokens.is_empty() { ptr::null() } else { s.tokens.as_ptr() }, n_tokens: s.tokens.len(), option: s.option as i32, reserved: 0 }).collect();
        let mut off = 0usize;
        let mut offs = Vec::with_capacity(rows.len());
        let mut out: Vec<_> = rows.iter().map(|&r| {
            let o = sys::rwkv_slot_output { logits: if r == 0 { ptr::null_mut() } else { unsafe { logits.ptr.add(off) } },
                                            logits_capacity_rows: r, n_rows: 0, n_consumed: 0 };
            offs.push(off);
            off += r * v;                         // consecutive pieces of one pinned block: one D2H copy
            o
        }).collect();
        check(unsafe { sys::rwkv_infer(self.raw, inp.as_ptr(), out.as_mut_ptr()) })?;     // fatal for the infer task, like `?` at run.rs:1143
        let mut res = Vec::with_capacity(out.len());
        for ((s, o), &at) in input.iter_mut().zip(&out).zip(&offs) {
            s.tokens.drain(..o.n_consumed);
            res.push(if o.n_rows == 0 { (0, 0) } else { (at, o.n_rows) });      // no pointer arithmetic on the null pointer of a row-less slot
        }
        Ok(res)
    }
    pub fn state_shape(&self) -> [usize; 4] { let mut s = [0usize; 4]; unsafe { sys::rwkv_state_shape(self.raw, s.as_mut_ptr()) }; s }
    pub fn state_init(&self) -> Result<Vec<f32>> {
        let mut v = vec![0f32; unsafe { sys::rwkv_state_len(self.raw) }];
        check(unsafe { sys::rwkv_state_init(self.raw, v.as_mut_ptr()) })?; Ok(v)
    }
    pub fn state_load(&self, slot: usize, data: &[f32]) -> Result<()> {
        if data.len() != unsafe { sys::rwkv_state_len(self.raw) } { return Err(Error { code: sys::RWKV_ERR_INVALID, message: "state tensor has the wrong size".into() }); }
        check(unsafe { sys::rwkv_state_load(self.raw, slot as i32, data.as_ptr()) })
    }
    pub fn state_back(&self, slot: usize) -> Result<Vec<f32>> {
        let mut v = vec![0f32; unsafe { sys::rwkv_state_len(self.raw) }];
        check(unsafe { sys::rwkv_state_back(self.raw, slot as i32, v.as_mut_ptr()) })?; Ok(v)
    }
    pub fn state_read(&self, slot: usize) -> Result<Arc<DeviceState>> {
        let mut p = ptr::null_mut();
        check(unsafe { sys::rwkv_state_read(self.raw, slot as i32, &mut p) })?; Ok(Arc::new(DeviceState(p)))
    }
    pub fn state_write(&self, slot: usize, snap: &DeviceState) -> Result<()> { check(unsafe { sys::rwkv_state_write(self.raw, slot as i32, snap.0) }) }
    /// WKV rows one layer owns in the state: `head_size` (64), for a V4 model its three rows aa / bb / pp
    pub fn layer_rows(&self) -> usize { if self.info.version == sys::RWKV_V4 { 3 } else { self.info.head_size as usize } }
    /// `/embeddings` (docs/doc-api/openai.md:376-437): one layer's WKV rows `[layer_rows][num_emb]`
    pub fn state_back_layer(&self, slot: usize, layer: usize) -> Result<Vec<f32>> {
        let mut v = vec![0f32; self.layer_rows() * self.info.num_emb as usize];
        check(unsafe { sys::rwkv_state_back_layer(self.raw, slot as i32, layer as i32, v.as_mut_ptr()) })?; Ok(v)
    }
    /// The same rows, not waited for: they land in the pinned block at float offset `at` and are valid after the copy stream has been
    /// waited for.  The slot may take its next request at once — a finished document's read-back overlaps the prefill of the following
    /// ones.  Soundness: while a device-to-host copy is in flight the block must be neither read nor freed, and a `&mut` argument alone
    /// does not say that (its borrow ends when the call returns).  So the call hands back a `PendingRows` guard that KEEPS the mutable
    /// borrow of `dst` (and a borrow of the engine): safe code cannot touch, move or drop the block until the guard is consumed by
    /// `PendingRows::sync()` — and dropping the guard without calling it waits too.  Several read-backs into ONE block go through
    /// `PendingRows::also` (disjoint ranges are checked), so the borrow is still held exactly once.
    pub fn state_back_layer_async<'a>(&'a self, slot: usize, layer: usize, dst: &'a mut PinnedLogits, at: usize) -> Result<PendingRows<'a>> {
        let mut p = PendingRows { rt: self, dst, ranges: Vec::new(), waited: false };
        p.issue(slot, layer, at)?;
        Ok(p)
    }
    /// waits for every pending `state_back_layer_async` (what `PendingRows::sync` calls; harmless when nothing is pending)
    pub fn state_sync(&self) -> Result<()> { check(unsafe { sys::rwkv_state_sync(self.raw) }) }
    /// `vN::read_state` (lib.rs:378-389); `Error.code == RWKV_ERR_NO_STATE` <-> the warning at lib.rs:442
    pub fn read_init_state(&self, st: &[u8]) -> Result<Vec<f32>> {
        let mut v = vec![0f32; unsafe { sys::rwkv_state_len(self.raw) }];
        check(unsafe { sys::rwkv_read_init_state(self.raw, st.as_ptr(), st.len(), v.as_mut_ptr()) })?; Ok(v)
    }
    /// `softmax::softmax(&context, Vec<TensorCpu>)` (run.rs:1179), in place; call from the softmax task's thread
    pub fn softmax(&self, rows: &mut [Vec<f32>]) -> Result<()> {
        let inp: Vec<*const f32> = rows.iter().map(|r| r.as_ptr()).collect();
        let out: Vec<*mut f32> = rows.iter_mut().map(|r| r.as_mut_ptr()).collect();
        check(unsafe { sys::rwkv_softmax(self.raw, inp.as_ptr(), out.as_ptr(), rows.len()) })
    }
    /// `rwkv_score_rows`: ln softmax(rows[i])[targets[i]] on the device (`sys::RWKV_SCORE_SKIP` -> NaN), one float per row back — the `head`
    /// term of Choose (run.rs:971-972).  Call from the softmax task's thread.
    pub fn score_rows(&self, rows: &[Vec<f32>], targets: &[u32]) -> Result<Vec<f32>> {
        let v = self.info.num_vocab as usize;
        if rows.len() != targets.len() || rows.iter().any(|r| r.len() != v) {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "score_rows: one target per row, num_vocab values per row".into() });
        }
        let inp: Vec<*const f32> = rows.iter().map(|r| r.as_ptr()).collect();
        let mut out = vec![f32::NAN; rows.len()];
        check(unsafe { sys::rwkv_score_rows(self.raw, inp.as_ptr(), targets.as_ptr(), out.as_mut_ptr(), rows.len()) })?;
        Ok(out)
    }
    /// `rwkv_infer_score`: one step like `infer`, for slots that are scored instead of read (perplexity run.rs:699-755, Choose run.rs:936-982).
    /// `targets[b]` is `None` (slot b has no tokens, or rides state-only with `OutputOption::None`) or one target per pending token of
    /// slot b: `targets[b][i]` (a token id or `sys::RWKV_SCORE_SKIP`) is scored on the row that consuming `tokens[b][i]` produces.  Tokens
    /// and targets are drained by what the call consumed; returns per slot the ln-probabilities of the consumed rows (NaN where skipped).
    pub fn infer_score(&self, input: &mut [SlotInput], targets: &mut [Option<Vec<u32>>]) -> Result<Vec<Vec<f32>>> {
        if input.len() != self.max_batch || targets.len() != self.max_batch {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("infer_score: {} slot inputs, {} target lists for max_batch {}", input.len(), targets.len(), self.max_batch) });
        }
        if input.iter().zip(targets.iter()).any(|(s, t)| t.as_ref().map_or(false, |t| t.len() != s.tokens.len())) {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "infer_score: a scored slot needs one target per pending token".into() });
        }
        let inp: Vec<_> = input.iter().map(|s| sys::rwkv_slot_input {
            tokens: if s.tokens.is_empty() { ptr::null() } else { s.tokens.as_ptr() }, n_tokens: s.tokens.len(), option: s.option as i32, reserved: 0 }).collect();
        let mut out: Vec<Vec<f32>> = targets.iter().map(|t| vec![f32::NAN; t.as_ref().map_or(0, |t| t.len().min(self.token_chunk_size))]).collect();
        let tp: Vec<*const u32> = targets.iter().map(|t| match t { Some(t) if !t.is_empty() => t.as_ptr(), _ => ptr::null() }).collect();
        let op: Vec<*mut f32> = out.iter_mut().map(|o| if o.is_empty() { ptr::null_mut() } else { o.as_mut_ptr() }).collect();
        let mut consumed = vec![0usize; self.max_batch];
        check(unsafe { sys::rwkv_infer_score(self.raw, inp.as_ptr(), tp.as_ptr(), op.as_ptr(), consumed.as_mut_ptr()) })?;
        for (((s, t), o), &n) in input.iter_mut().zip(targets.iter_mut()).zip(out.iter_mut()).zip(&consumed) {
            s.tokens.drain(..n);
            if let Some(t) = t { t.drain(..n); o.truncate(n); }
        }
        Ok(out)
    }
    /// `rwkv_topn_rows`: the `n` most likely tokens of every row and their ln-probabilities on the device, `[rows][n]` each: logits
    /// descending, ties to the lower id; `sys::RWKV_TOPN_NONE` / -inf where a row has fewer than n entries above -inf, `RWKV_TOPN_NONE` /
    /// NaN on a row holding +inf or NaN.  Every logp is `score_rows`' value for that row and id.  Call from the softmax task's thread.
    pub fn topn_rows(&self, rows: &[Vec<f32>], n: usize) -> Result<(Vec<u32>, Vec<f32>)> {
        let v = self.info.num_vocab as usize;
        if rows.iter().any(|r| r.len() != v) || n < 1 || n > sys::RWKV_TOPN_MAX as usize {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "topn_rows: num_vocab values per row, n in 1..=RWKV_TOPN_MAX".into() });
        }
        let inp: Vec<*const f32> = rows.iter().map(|r| r.as_ptr()).collect();
        let (mut ids, mut lp) = (vec![sys::RWKV_TOPN_NONE; rows.len() * n], vec![f32::NAN; rows.len() * n]);
        check(unsafe { sys::rwkv_topn_rows(self.raw, inp.as_ptr(), n as i32, ids.as_mut_ptr(), lp.as_mut_ptr(), rows.len()) })?;
        Ok((ids, lp))
    }
    /// `rwkv_infer_topn`: one step like `infer`, with top-n lists instead of rows.  Every slot that has tokens and an option other than
    /// `OutputOption::None` lists and keeps its option (`Last`: one list when the call exhausts its tokens, `Full`: one per consumed
    /// token).  `targets[b]` is `None` or one target per pending token of a `Full` slot (a token id or `sys::RWKV_SCORE_SKIP`): the realised
    /// token's ln-probability, exactly `infer_score`'s, comes back beside the alternatives.  Tokens and targets are drained by what the call
    /// consumed; returns one `TopLists` per slot (`rows == 0` for a slot that listed nothing).
    pub fn infer_topn(&self, input: &mut [SlotInput], n: usize, targets: &mut [Option<Vec<u32>>]) -> Result<Vec<TopLists>> {
        if input.len() != self.max_batch || targets.len() != self.max_batch || n < 1 || n > sys::RWKV_TOPN_MAX as usize {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("infer_topn: {} slot inputs, {} target lists for max_batch {}, n = {}", input.len(), targets.len(), self.max_batch, n) });
        }
        if input.iter().zip(targets.iter()).any(|(s, t)| t.as_ref().map_or(false, |t| t.len() != s.tokens.len())) {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "infer_topn: a scored slot needs one target per pending token".into() });
        }
        let inp: Vec<_> = input.iter().map(|s| sys::rwkv_slot_input {
            tokens: if s.tokens.is_empty() { ptr::null() } else { s.tokens.as_ptr() }, n_tokens: s.tokens.len(), option: s.option as i32, reserved: 0 }).collect();
        let mut out: Vec<TopLists> = input.iter().zip(targets.iter()).map(|(s, t)| {
            let rows = if s.tokens.is_empty() || s.option as i32 == sys::RWKV_OPTION_NONE { 0 }
                       else if s.option as i32 == sys::RWKV_OPTION_FULL { s.tokens.len().min(self.token_chunk_size) } else { 1 };
            TopLists { n, rows, ids: vec![sys::RWKV_TOPN_NONE; rows * n], logp: vec![f32::NAN; rows * n],
                       tok_logp: if t.is_some() { vec![f32::NAN; rows] } else { Vec::new() } }
        }).collect();
        let ip: Vec<*mut u32> = out.iter_mut().map(|o| if o.rows == 0 { ptr::null_mut() } else { o.ids.as_mut_ptr() }).collect();
        let lp: Vec<*mut f32> = out.iter_mut().map(|o| if o.rows == 0 { ptr::null_mut() } else { o.logp.as_mut_ptr() }).collect();
        let tp: Vec<*const u32> = targets.iter().map(|t| match t { Some(t) if !t.is_empty() => t.as_ptr(), _ => ptr::null() }).collect();
        let op: Vec<*mut f32> = out.iter_mut().map(|o| if o.tok_logp.is_empty() { ptr::null_mut() } else { o.tok_logp.as_mut_ptr() }).collect();
        let (mut n_rows, mut consumed) = (vec![0usize; self.max_batch], vec![0usize; self.max_batch]);
        check(unsafe { sys::rwkv_infer_topn(self.raw, inp.as_ptr(), n as i32, ip.as_ptr(), lp.as_ptr(), tp.as_ptr(), op.as_ptr(), n_rows.as_mut_ptr(), consumed.as_mut_ptr()) })?;
        for ((((s, t), o), &r), &k) in input.iter_mut().zip(targets.iter_mut()).zip(out.iter_mut()).zip(&n_rows).zip(&consumed) {
            s.tokens.drain(..k);
            if let Some(t) = t { t.drain(..k); }
            o.rows = r; o.ids.truncate(r * n); o.logp.truncate(r * n);
            if !o.tok_logp.is_empty() { o.tok_logp.truncate(r); }
        }
        Ok(out)
    }
    /// Arm `slot` for device-resident sampled generation (rwkv_gen_arm): the decode loop of `process` (run.rs:788-1020) with `sample()`
    /// (run.rs:664-697) and the sampler state machine (sampler/*.rs) on the device.  The slot's state is what the prompt left.
    pub fn gen_arm(&self, slot: usize, p: &GenParams) -> Result<()> { self.gen_arm_with(slot, p, None) }
    /// Admission (rwkv_gen_arm_prompt, run.rs:788-832 without leaving the loop): arm `slot` with the not-yet-consumed tail of its
    /// prompt.  `p.penalties` is the map `Sampler::init` left (before any draw), `p.first_token` is ignored: the following `gen_run`
    /// steps prefill next to the running slots' decode rows and draw the first token on the device (draw 0 of (seed, stream)).
    pub fn gen_arm_prompt(&self, slot: usize, tokens: &[u32], p: &GenParams) -> Result<()> { self.gen_arm_with(slot, p, Some(tokens)) }
    /// prompt tokens of `slot` the resident steps have not consumed yet (rwkv_gen_prompt_left)
    pub fn gen_prompt_left(&self, slot: usize) -> Result<usize> {
        let mut left = 0usize;
        check(unsafe { sys::rwkv_gen_prompt_left(self.raw, slot as i32, &mut left) })?; Ok(left)
    }
    /// `gen_arm_prompt` for a prompt that is wholly cached (rwkv_gen_arm_item, run.rs:809-810): the slot's state becomes the item's and its
    /// first token is drawn on the device from the item's row, draw 0 of (seed, stream), in a first step that consumes nothing.
    pub fn gen_arm_item(&self, slot: usize, item: &GenItem, p: &GenParams) -> Result<()> { self.gen_arm_from(slot, p, None, Some(item)) }
    /// What an armed, unfinished slot keeps for the prefix cache (rwkv_gen_set_capture), between runs; an empty slice clears it.
    pub fn gen_set_capture(&self, slot: usize, what: &[GenCapture]) -> Result<()> {
        check(unsafe { sys::rwkv_gen_set_capture(self.raw, slot as i32, what.iter().fold(0u32, |m, &w| m | w as u32)) })
    }
    /// The slot's captured item (rwkv_gen_take_item): `Prompt` once the run that exhausted the prompt has returned, `Finish` once the slot
    /// has finished; each once.
    pub fn gen_take_item(&self, slot: usize, which: GenCapture) -> Result<std::sync::Arc<GenItem>> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_gen_take_item(self.raw, slot as i32, which as u32, &mut raw) })?;
        Ok(std::sync::Arc::new(GenItem(raw)))
    }
    /// (state in the layout of `state_back`, row of num_vocab floats) of an item on the host (rwkv_gen_item_back), bit for bit
    pub fn gen_item_back(&self, item: &GenItem) -> Result<(Vec<f32>, Vec<f32>)> {
        let (mut state, mut row) = (vec![0f32; unsafe { sys::rwkv_state_len(self.raw) }], vec![0f32; self.info.num_vocab as usize]);
        check(unsafe { sys::rwkv_gen_item_back(self.raw, item.0, state.as_mut_ptr(), row.as_mut_ptr()) })?;
        Ok((state, row))
    }
    /// an item of this engine's device from what `gen_item_back` returned (rwkv_gen_item_from_host)
    pub fn gen_item_from_host(&self, state: &[f32], row: &[f32]) -> Result<std::sync::Arc<GenItem>> {
        if state.len() != unsafe { sys::rwkv_state_len(self.raw) } || row.len() != self.info.num_vocab as usize {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "gen_item_from_host: state or row has the wrong length".into() });
        }
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_gen_item_from_host(self.raw, state.as_ptr(), row.as_ptr(), &mut raw) })?;
        Ok(std::sync::Arc::new(GenItem(raw)))
    }
    /// the item's state into `slot` (rwkv_state_write of rwkv_gen_item_state): a PARTIAL prefix hit, continued with `gen_arm_prompt`
    pub fn gen_item_state_to(&self, item: &GenItem, slot: usize) -> Result<()> {
        check(unsafe { sys::rwkv_state_write(self.raw, slot as i32, sys::rwkv_gen_item_state(item.0)) })
    }
    fn gen_arm_with(&self, slot: usize, p: &GenParams, prompt: Option<&[u32]>) -> Result<()> { self.gen_arm_from(slot, p, prompt, None) }
    fn gen_arm_from(&self, slot: usize, p: &GenParams, prompt: Option<&[u32]>, item: Option<&GenItem>) -> Result<()> {
        let (pt, pv): (Vec<u32>, Vec<f32>) = p.penalties.iter().copied().unzip();
        let (bt, bv): (Vec<u32>, Vec<f32>) = p.bias.iter().copied().unzip();
        let raw = sys::rwkv_gen_params {
            first_token: p.first_token, max_tokens: p.max_tokens as i32, kind: p.kind as i32, top_p: p.top_p, top_k: p.top_k.min(i32::MAX as usize) as i32,
            temperature: p.temperature, tau: p.tau, presence_penalty: p.presence_penalty, frequency_penalty: p.frequency_penalty,
            penalty_decay: p.penalty_decay, miro_target: p.miro_target, miro_rate: p.miro_rate,
            penalty_tokens: pt.as_ptr(), penalty_values: pv.as_ptr(), n_penalty: pt.len(),
            bias_tokens: bt.as_ptr(), bias_values: bv.as_ptr(), n_bias: bt.len(),
            stop_tokens: p.stop_tokens.as_ptr(), n_stop: p.stop_tokens.len(), allow: ptr::null(),
            seed: p.seed, stream: p.stream, reserved: if p.top_k > 256 { sys::RWKV_GEN_WIDE_TOP_K } else { 0 },
        };
        match (prompt, item) {
            (_, Some(it)) => check(unsafe { sys::rwkv_gen_arm_item(self.raw, slot as i32, it.0, &raw) }),
            (None, None) => check(unsafe { sys::rwkv_gen_arm(self.raw, slot as i32, &raw) }),
            (Some(t), None) => check(unsafe { sys::rwkv_gen_arm_prompt(self.raw, slot as i32, t.as_ptr(), t.len(), &raw) }),
        }
    }
    pub fn gen_disarm(&self, slot: usize) -> Result<()> { check(unsafe { sys::rwkv_gen_disarm(self.raw, slot as i32) }) }
    /// `tokenizer.decode(&[token])` for every id (rwkv_gen_set_token_bytes, run.rs:856): `None` is an id that is not in the vocabulary —
    /// the decode error of run.rs:858-862, an empty word and a stop.  What the device matches stop strings over.
    pub fn gen_set_token_bytes(&self, tokens: &[Option<&[u8]>]) -> Result<()> {
        let lens: Vec<i32> = tokens.iter().map(|t| t.map_or(-1, |b| b.len() as i32)).collect();
        let bytes: Vec<u8> = tokens.iter().flat_map(|t| t.unwrap_or(&[]).iter().copied()).collect();
        check(unsafe { sys::rwkv_gen_set_token_bytes(self.raw, bytes.as_ptr(), lens.as_ptr(), lens.len()) })
    }
    /// `GenerateRequest::stop` of an armed, unfinished slot (rwkv_gen_set_stops, run.rs:899-932), matched on the device inside the step;
    /// `tail` is `context.buffer` as the caller's own matcher holds it after the tokens it handled itself.  An empty list clears them.
    pub fn gen_set_stops(&self, slot: usize, stops: &[&[u8]], tail: &[u8]) -> Result<()> {
        let strs: Vec<*const u8> = stops.iter().map(|s| s.as_ptr()).collect();
        let lens: Vec<usize> = stops.iter().map(|s| s.len()).collect();
        let raw = sys::rwkv_gen_stops { strs: strs.as_ptr(), lens: lens.as_ptr(), n: stops.len(), tail: tail.as_ptr(), n_tail: tail.len() };
        check(unsafe { sys::rwkv_gen_set_stops(self.raw, slot as i32, &raw) })
    }
    /// the slot's matcher buffer as it stands (rwkv_gen_stop_tail; `buffer = tail`, run.rs:1010): what a caller that resumes per token starts from
    pub fn gen_stop_tail(&self, slot: usize) -> Result<Vec<u8>> {
        let mut out = vec![0u8; sys::RWKV_GEN_STOP_BUF];
        let mut len = 0usize;
        check(unsafe { sys::rwkv_gen_stop_tail(self.raw, slot as i32, out.as_mut_ptr(), out.len(), &mut len) })?;
        out.truncate(len);
        Ok(out)
    }
    /// The format constraint of an armed, unfinished slot (rwkv_gen_set_constraint): a byte-level DFA masked, advanced and halted on the
    /// device — the `Formatter` trait (sampler/bnf.rs:34-48) for REGULAR constraints; kbnf's grammars stay on the host.  `state` is
    /// `dfa.start()` after `gen_arm_prompt`, after `gen_arm` the state behind `first_token`.  `None` clears the constraint.
    pub fn gen_set_constraint(&self, slot: usize, dfa: Option<&Dfa>, state: i32, halt: DfaHalt) -> Result<()> {
        let raw = dfa.map_or(ptr::null(), |d| d.raw as *const sys::rwkv_dfa);
        check(unsafe { sys::rwkv_gen_set_constraint(self.raw, slot as i32, raw, state, halt as i32) })
    }
    /// the automaton state behind every token the slot has emitted (rwkv_gen_constraint_state): what the per-token path goes on from
    pub fn gen_constraint_state(&self, slot: usize) -> Result<i32> {
        let mut state = 0i32;
        check(unsafe { sys::rwkv_gen_constraint_state(self.raw, slot as i32, &mut state) })?; Ok(state)
    }
    /// The stack constraint of an armed, unfinished slot (rwkv_gen_set_pda): a byte automaton with a return-state stack (`Pda::json` for
    /// "answer in JSON") masked, committed and halted on the device.  `(state, stack)` is `(pda.start(), &[])` after `gen_arm_prompt`, the
    /// caller's own configuration after `gen_arm` or a hand-over.  `None` clears it.  A slot holds a `Dfa` or a `Pda`, not both.
    pub fn gen_set_pda(&self, slot: usize, pda: Option<&Pda>, state: i32, stack: &[u16], halt: PdaHalt) -> Result<()> {
        let raw = pda.map_or(ptr::null(), |p| p.raw as *const sys::rwkv_pda);
        check(unsafe { sys::rwkv_gen_set_pda(self.raw, slot as i32, raw, state, stack.as_ptr(), stack.len() as i32, halt as i32) })
    }
    /// the configuration behind every token the slot has emitted (rwkv_gen_pda_config): what the per-token path goes on from
    pub fn gen_pda_config(&self, slot: usize) -> Result<(i32, Vec<u16>)> {
        let (mut state, mut depth) = (0i32, 0i32);
        let mut stack = vec![0u16; sys::RWKV_PDA_MAX_DEPTH];
        check(unsafe { sys::rwkv_gen_pda_config(self.raw, slot as i32, &mut state, stack.as_mut_ptr(), stack.len(), &mut depth) })?;
        stack.truncate(depth.max(0) as usize);
        Ok((state, stack))
    }
    /// Up to `n_steps` tokens for every armed, unfinished slot with no host turn-around (rwkv_gen_run).  When it returns a slot's
    /// state has consumed everything it emitted except the last token (what run.rs:990-1005 backs up at a stop).
    pub fn gen_run(&self, n_steps: usize) -> Result<Generated> {
        let mut g = Generated { tokens: vec![u32::MAX; n_steps * self.max_batch], probs: vec![f32::NAN; n_steps * self.max_batch],
                                n_emitted: vec![0; self.max_batch], finish: vec![0; self.max_batch] };
        check(unsafe { sys::rwkv_gen_run(self.raw, n_steps as i32, g.tokens.as_mut_ptr(), g.probs.as_mut_ptr(), g.n_emitted.as_mut_ptr(), g.finish.as_mut_ptr()) })?;
        Ok(g)
    }
    /// An armed, unfinished slot lists its `n` (0 ..= RWKV_TOPN_MAX; 0 = off) most likely tokens of the RAW model row — before penalties,
    /// bias, temperature and any constraint mask — with every token it emits from now on (rwkv_gen_set_topn).  Re-arming resets it.
    pub fn gen_set_topn(&self, slot: usize, n: usize) -> Result<()> { check(unsafe { sys::rwkv_gen_set_topn(self.raw, slot as i32, n as i32) }) }
    /// `gen_run` with the lists (rwkv_gen_run_topn): `n_top` (>= every armed slot's n) is the stride of `top_ids` / `top_logp`.
    pub fn gen_run_topn(&self, n_steps: usize, n_top: usize) -> Result<GeneratedTop> {
        let cells = n_steps * self.max_batch;
        let mut g = Generated { tokens: vec![u32::MAX; cells], probs: vec![f32::NAN; cells], n_emitted: vec![0; self.max_batch], finish: vec![0; self.max_batch] };
        let (mut tok_logp, mut top_ids, mut top_logp) = (vec![f32::NAN; cells], vec![sys::RWKV_TOPN_NONE; cells * n_top], vec![f32::NAN; cells * n_top]);
        check(unsafe { sys::rwkv_gen_run_topn(self.raw, n_steps as i32, g.tokens.as_mut_ptr(), g.probs.as_mut_ptr(), g.n_emitted.as_mut_ptr(), g.finish.as_mut_ptr(),
                                              n_top as i32, tok_logp.as_mut_ptr(), top_ids.as_mut_ptr(), top_logp.as_mut_ptr()) })?;
        Ok(GeneratedTop { run: g, n_top, tok_logp, top_ids, top_logp })
    }
}

#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)] pub enum DfaHalt { #[default] Final = 0, Accept = 1 }
/// A byte-level DFA (rwkv_dfa): state 0 is dead, `compile` takes the anchored regex dialect of include/rwkv_abi.h, `from_table` any
/// compiler's table.  Immutable; host only.  Not kbnf: regular constraints only.
#[derive(Debug)]
pub struct Dfa { raw: *mut sys::rwkv_dfa }
unsafe impl Send for Dfa {}
unsafe impl Sync for Dfa {}
impl Drop for Dfa { fn drop(&mut self) { unsafe { sys::rwkv_dfa_free(self.raw) } } }
impl Dfa {
    pub fn compile(pattern: &[u8]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_dfa_compile(pattern.as_ptr(), pattern.len(), &mut raw) })?; Ok(Self { raw })
    }
    pub fn from_table(trans: &[u16], accepting: &[u8], start: i32) -> Result<Self> {
        if trans.len() != accepting.len() * 256 {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "Dfa::from_table: 256 transitions per state".into() });
        }
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_dfa_from_table(trans.as_ptr(), accepting.as_ptr(), accepting.len() as i32, start, &mut raw) })?; Ok(Self { raw })
    }
    pub fn num_states(&self) -> i32 { unsafe { sys::rwkv_dfa_num_states(self.raw) } }
    pub fn start(&self) -> i32 { unsafe { sys::rwkv_dfa_start(self.raw) } }
    /// the state `bytes` behind `state` (0 once the walk died)
    pub fn walk(&self, state: i32, bytes: &[u8]) -> Result<i32> {
        let mut next = 0i32;
        check(unsafe { sys::rwkv_dfa_walk(self.raw, state, bytes.as_ptr(), bytes.len(), &mut next) })?; Ok(next)
    }
    /// `Formatter::transform` on the host (rwkv_dfa_allow): the mask `SampleParams::allow` takes; `tokens` as for `gen_set_token_bytes`
    pub fn allow(&self, state: i32, tokens: &[Option<&[u8]>], num_vocab: usize) -> Result<Vec<u8>> {
        let lens: Vec<i32> = tokens.iter().map(|t| t.map_or(-1, |b| b.len() as i32)).collect();
        let bytes: Vec<u8> = tokens.iter().flat_map(|t| t.unwrap_or(&[]).iter().copied()).collect();
        let mut out = vec![0u8; num_vocab];
        check(unsafe { sys::rwkv_dfa_allow(self.raw, state, bytes.as_ptr(), lens.as_ptr(), lens.len(), out.as_mut_ptr(), num_vocab) })?; Ok(out)
    }
}
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)] pub enum PdaHalt { #[default] Final = 0, Accept = 1 }
/// A byte automaton with a return-state stack (rwkv_pda): state 0 is dead, a configuration is (state, stack).  `json` is RFC 8259
/// (`flags`: `RWKV_PDA_JSON_OBJECT | RWKV_PDA_JSON_COMPACT`), `from_table` takes any compiler's two planes.  Immutable; host only.
/// Not kbnf: what a return-state stack expresses, nested brackets above all.
#[derive(Debug)]
pub struct Pda { raw: *mut sys::rwkv_pda }
unsafe impl Send for Pda {}
unsafe impl Sync for Pda {}
impl Drop for Pda { fn drop(&mut self) { unsafe { sys::rwkv_pda_free(self.raw) } } }
impl Pda {
    pub fn json(flags: u32, max_depth: i32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_pda_json(flags, max_depth, &mut raw) })?; Ok(Self { raw })
    }
    pub fn from_table(next: &[u16], act: &[u16], accepting: &[u8], start: i32, max_depth: i32) -> Result<Self> {
        if next.len() != accepting.len() * 256 || act.len() != next.len() {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: "Pda::from_table: two planes of 256 entries per state".into() });
        }
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rwkv_pda_from_table(next.as_ptr(), act.as_ptr(), accepting.as_ptr(), accepting.len() as i32, start, max_depth, &mut raw) })?;
        Ok(Self { raw })
    }
    pub fn num_states(&self) -> i32 { unsafe { sys::rwkv_pda_num_states(self.raw) } }
    pub fn start(&self) -> i32 { unsafe { sys::rwkv_pda_start(self.raw) } }
    pub fn max_depth(&self) -> i32 { unsafe { sys::rwkv_pda_max_depth(self.raw) } }
    /// the configuration `bytes` behind `(state, stack)` (state 0 once the walk died)
    pub fn walk(&self, state: i32, stack: &[u16], bytes: &[u8]) -> Result<(i32, Vec<u16>)> {
        let (mut q, mut depth) = (0i32, 0i32);
        let mut out = vec![0u16; sys::RWKV_PDA_MAX_DEPTH];
        check(unsafe { sys::rwkv_pda_walk(self.raw, state, stack.as_ptr(), stack.len() as i32, bytes.as_ptr(), bytes.len(), &mut q, out.as_mut_ptr(), &mut depth) })?;
        out.truncate(depth.max(0) as usize);
        Ok((q, out))
    }
    /// `Formatter::transform` on the host (rwkv_pda_allow): the mask `SampleParams::allow` takes; `tokens` as for `gen_set_token_bytes`
    pub fn allow(&self, state: i32, stack: &[u16], tokens: &[Option<&[u8]>], num_vocab: usize) -> Result<Vec<u8>> {
        let lens: Vec<i32> = tokens.iter().map(|t| t.map_or(-1, |b| b.len() as i32)).collect();
        let bytes: Vec<u8> = tokens.iter().flat_map(|t| t.unwrap_or(&[]).iter().copied()).collect();
        let mut out = vec![0u8; num_vocab];
        check(unsafe { sys::rwkv_pda_allow(self.raw, state, stack.as_ptr(), stack.len() as i32, bytes.as_ptr(), lens.as_ptr(), lens.len(), out.as_mut_ptr(), num_vocab) })?;
        Ok(out)
    }
}
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)] pub enum SamplerKind { #[default] Nucleus = 0, Typical = 1, Mirostat = 2 }
/// `rwkv_gen_params`: sampler settings (nucleus.rs:13-26, typical.rs:11-24, mirostat.rs:11-36), the penalty map `init` left over the
/// prompt (nucleus.rs:49-59), `GenerateRequest::bias` (run.rs:681-683), stop tokens (token 0 always stops, run.rs:855) and the
/// (seed, stream) of the counter-based uniform draw (`gen_uniform`).  `top_k` is any `usize`, as in the reference: above 256 the slot is
/// armed with `RWKV_GEN_WIDE_TOP_K` and sampled by the wide kernel; Mirostat is exact for every `max_surprise`.
#[derive(Clone, Debug, Default)]
pub struct GenParams {
    pub first_token: u32, pub max_tokens: usize, pub kind: SamplerKind, pub top_p: f32, pub top_k: usize, pub temperature: f32, pub tau: f32,
    pub presence_penalty: f32, pub frequency_penalty: f32, pub penalty_decay: f32, pub miro_target: f32, pub miro_rate: f32,
    pub penalties: Vec<(u32, f32)>, pub bias: Vec<(u32, f32)>, pub stop_tokens: Vec<u32>, pub seed: u64, pub stream: u32,
}
/// what `Engine::gen_run` returns: `tokens` / `probs` are [n_steps][max_batch] (u32::MAX / NaN where a slot emitted nothing),
/// `n_emitted` counts this call's tokens per slot, `finish` is RWKV_GEN_RUNNING / _STOP / _LENGTH / _HANDBACK
#[derive(Clone, Debug)]
pub struct Generated { pub tokens: Vec<u32>, pub probs: Vec<f32>, pub n_emitted: Vec<i32>, pub finish: Vec<i32> }
/// what `Engine::gen_run_topn` returns beside `gen_run`'s: `tok_logp` [n_steps][max_batch] is the emitted token's raw ln-probability (NaN where
/// nothing was emitted or the slot lists nothing), `top_ids` / `top_logp` [n_steps][max_batch][n_top] the lists (`sys::RWKV_TOPN_NONE` / -inf
/// behind a slot's own n, `RWKV_TOPN_NONE` / NaN where nothing was emitted)
#[derive(Clone, Debug)]
pub struct GeneratedTop { pub run: Generated, pub n_top: usize, pub tok_logp: Vec<f32>, pub top_ids: Vec<u32>, pub top_logp: Vec<f32> }
/// draw `step` of (seed, stream): pure host function (rwkv_gen_uniform)
pub fn gen_uniform(seed: u64, stream: u32, step: u32) -> f32 {
    let mut u = 0f32;
    unsafe { sys::rwkv_gen_uniform(seed, stream, step, 1, &mut u) };
    u
}

/// Read-backs in flight into one pinned block (`Engine::state_back_layer_async`).  Holds the block's mutable borrow until the copy
/// stream has been waited for: `sync()` gives the block back; `Drop` waits as well, so no path — early return, `?`, panic unwinding —
/// lets the block be read or freed under the DMA.  `std::mem::forget(guard)` is the one safe-code path that ends the borrow without the wait
/// (leaking a guard is safe Rust): `PinnedLogits` therefore counts the read-backs in flight into it (`in_flight`) and its own `Drop` and
/// `as_slice` wait on the engine's copy stream while the count is non-zero.
pub struct PendingRows<'a> {
    rt: &'a Engine,
    dst: &'a mut PinnedLogits,
    ranges: Vec<(usize, usize)>,
    waited: bool,
}
impl<'a> PendingRows<'a> {
    fn issue(&mut self, slot: usize, layer: usize, at: usize) -> Result<()> {
        let n = self.rt.layer_rows() * self.rt.info.num_emb as usize;
        let end = match at.checked_add(n) { Some(e) if e <= self.dst.floats => e, _ => {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("pinned block holds {} floats, rows need {}..{}", self.dst.floats, at, at.saturating_add(n)) }) } };
        if self.ranges.iter().any(|&(a, b)| at < b && a < end) {
            return Err(Error { code: sys::RWKV_ERR_INVALID, message: format!("rows {}..{} overlap a read-back already in flight into this block", at, end) });
        }
        check(unsafe { sys::rwkv_state_back_layer_async(self.rt.raw, slot as i32, layer as i32, self.dst.ptr.add(at)) })?;
        self.ranges.push((at, end));
        self.dst.in_flight += 1;
        Ok(())
    }
    /// one more slot's rows into the same block (a disjoint range), still under the one borrow
    pub fn also(&mut self, slot: usize, layer: usize, at: usize) -> Result<()> { self.issue(slot, layer, at) }
    /// wait for the copies; the block is the caller's again
    /// On `Err` the copies may NOT have completed: the guard is dropped at the end of this call with `waited` still false, so its `Drop` waits once
    /// more before the borrow ends, and the block is not handed back.
    pub fn sync(mut self) -> Result<&'a mut PinnedLogits> {
        self.rt.state_sync()?;
        self.waited = true;
        self.dst.in_flight -= self.ranges.len();
        // SAFETY: `self` is consumed and its Drop (below) does nothing once `waited`; the reference is re-borrowed for the original lifetime
        let dst: *mut PinnedLogits = &mut *self.dst;                 // a reborrow, not a move out of a `Drop` type
        Ok(unsafe { &mut *dst })
    }
}
impl Drop for PendingRows<'_> {
    /// waits; only a SUCCESSFUL wait releases the block's in-flight count (after a failed one the block stays unreadable and is leaked on drop)
    fn drop(&mut self) { if !self.waited && self.rt.state_sync().is_ok() { self.dst.in_flight -= self.ranges.len(); } }
}

/// `Tokenizer` (lib.rs:375; run.rs:157-168, 856; sampler/bnf.rs:14-27)
#[derive(Debug)]                       // `RuntimeInfo`, `ThreadRequest` and `CoreRuntime` derive Debug over an `Arc<Tokenizer>` (lib.rs:80, 116; run.rs:374)
pub struct Tokenizer(*mut sys::rwkv_tokenizer);
unsafe impl Send for Tokenizer {}
unsafe impl Sync for Tokenizer {}
impl Drop for Tokenizer { fn drop(&mut self) { unsafe { sys::rwkv_tokenizer_destroy(self.0) } } }
impl Tokenizer {
    pub fn new(vocab_json: &str) -> Result<Self> {
        let mut p = ptr::null_mut();
        check(unsafe { sys::rwkv_tokenizer_create(vocab_json.as_ptr() as *const _, vocab_json.len(), &mut p) })?; Ok(Self(p))
    }
    pub fn encode(&self, text: &[u8]) -> Result<Vec<u32>> {
        let n = unsafe { sys::rwkv_tokenizer_encode(self.0, text.as_ptr(), text.len(), ptr::null_mut(), 0) };
        if n < 0 { return Err(Error { code: n as i32, message: "no matching token found".into() }); }
        let mut v = vec![0u32; n as usize];
        unsafe { sys::rwkv_tokenizer_encode(self.0, text.as_ptr(), text.len(), v.as_mut_ptr(), v.len()) }; Ok(v)
    }
    pub fn decode(&self, tokens: &[u32]) -> Result<Vec<u8>> {
        let n = unsafe { sys::rwkv_tokenizer_decode(self.0, tokens.as_ptr(), tokens.len(), ptr::null_mut(), 0) };
        if n < 0 { return Err(Error { code: n as i32, message: "token index out of range".into() }); }
        let mut v = vec![0u8; n as usize];
        unsafe { sys::rwkv_tokenizer_decode(self.0, tokens.as_ptr(), tokens.len(), v.as_mut_ptr(), v.len()) }; Ok(v)
    }
    /// `token_index_to_bytes` (bnf.rs:15)
    pub fn token_index_to_bytes(&self) -> Vec<Vec<u8>> {
        (0..unsafe { sys::rwkv_tokenizer_vocab_size(self.0) }.max(0) as u32).map(|i| {
            let n = unsafe { sys::rwkv_tokenizer_token_bytes(self.0, i, ptr::null_mut(), 0) };
            let mut v = vec![0u8; n.max(0) as usize];
            if n > 0 { unsafe { sys::rwkv_tokenizer_token_bytes(self.0, i, v.as_mut_ptr(), v.len()) }; }
            v
        }).collect()
    }
}

pub mod compat;
