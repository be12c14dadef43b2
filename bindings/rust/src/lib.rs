//! Safe wrappers over `sys.rs` for the entry points the bridge's verifier calls (INTEGRATION.md has the call-site table).
//! Not built in the repository this file lives in (no cargo there); kept next to the header it is generated from.
mod sys;
pub use sys::*;
use std::ffi::CStr;

pub struct Ctx(*mut mina_ctx);
unsafe impl Send for Ctx {}          // one context per worker thread; not Sync

#[derive(Debug)]
pub struct MinaError(pub i32, pub String);

fn check(rc: i32) -> Result<(), MinaError> {
    if rc == 0 { Ok(()) } else {
        let msg = unsafe { CStr::from_ptr(mina_last_error()) }.to_string_lossy().into_owned();
        Err(MinaError(rc, msg))
    }
}

impl Ctx {
    pub fn new(device: i32) -> Result<Self, MinaError> {
        let mut p = std::ptr::null_mut();
        check(unsafe { mina_ctx_create(device, &mut p) })?;
        Ok(Ctx(p))
    }
    /// `SRS::<G>::create(depth)` on the GPU (regenerates srs/vesta.srs / srs/pallas.srs point for point).
    pub fn srs_create(&mut self, curve: i32, depth: u32) -> Result<(), MinaError> {
        check(unsafe { mina_srs_create(self.0, curve, depth) })
    }
    /// openmina `accumulator_check` for `sg.len() / 64` proofs, one deterministic verdict each.
    pub fn accumulator_check_multi(&mut self, curve: i32, k: u32, prechallenges: &[u8], sg: &[u8]) -> Result<Vec<bool>, MinaError> {
        let n = sg.len() / 64;
        assert_eq!(prechallenges.len(), n * k as usize * 16);
        let mut v = vec![0u8; n];
        check(unsafe { mina_accumulator_check_multi(self.0, curve, k, n, prechallenges.as_ptr(), sg.as_ptr(), v.as_mut_ptr()) })?;
        Ok(v.into_iter().map(|b| b != 0).collect())
    }
    /// The protocol-state leg of this context's Proof-of-State jobs hashes each distinct state of a job once (off by default; no result changes).
    pub fn set_state_dedup(&mut self, on: bool) -> Result<(), MinaError> {
        check(unsafe { mina_ctx_set_state_dedup(self.0, on as i32) })
    }
    /// `SRS::verify` on a batch; the two RNG draws of upstream are explicit arguments.  Any failure is `false`.
    pub fn ipa_batch_check(&mut self, curve: i32, openings: &[mina_ipa_opening], rand_base: &[u8; 32], sg_rand_base: &[u8; 32]) -> bool {
        let mut v = 0u8;
        let rc = unsafe { mina_ipa_batch_check(self.0, curve, openings.len(), openings.as_ptr(), rand_base.as_ptr(), sg_rand_base.as_ptr(), &mut v) };
        rc == 0 && v == 1
    }
}

/// Stands where Aligned's `verify_mina_state_ffi` stands: the bytes of `bincode::serialize(&MinaStateProof)` / `(&MinaStatePubInputs)`
/// (core/src/aligned.rs:33-36).  Process-wide context, every failure is `false`.
/// NEVER COMPILED: this crate is generated from include/mina_verify.h and diffed against it (tests/test_abi.py); the image it was written in has no cargo.
/// Before calling it a drop-in, build it and link it under the caller of core/src/aligned.rs:31-58.
pub fn verify_mina_state(proof: &[u8], pub_input: &[u8]) -> bool {
    unsafe { mina_verify_state(proof.as_ptr(), proof.len(), pub_input.as_ptr(), pub_input.len()) }
}
/// Stands where `verify_account_inclusion_ffi` stands (core/src/aligned.rs:46-49); never compiled either (see above).
pub fn verify_account_inclusion(proof: &[u8], pub_input: &[u8]) -> bool {
    unsafe { mina_verify_account(proof.as_ptr(), proof.len(), pub_input.as_ptr(), pub_input.len()) }
}
/// Batch form: one GPU pipeline for all proofs, one verdict each.
pub fn verify_mina_state_batch(proofs: &[&[u8]], pub_inputs: &[&[u8]]) -> Vec<bool> {
    let n = proofs.len();
    let (pp, pl): (Vec<_>, Vec<_>) = proofs.iter().map(|p| (p.as_ptr(), p.len())).unzip();
    let (qp, ql): (Vec<_>, Vec<_>) = pub_inputs.iter().map(|p| (p.as_ptr(), p.len())).unzip();
    let mut v = vec![0u8; n];
    let rc = unsafe { mina_verify_state_batch(n, pp.as_ptr(), pl.as_ptr(), qp.as_ptr(), ql.as_ptr(), v.as_mut_ptr()) };
    v.into_iter().map(|b| rc == 0 && b == 1).collect()
}

impl Drop for Ctx {
    fn drop(&mut self) { unsafe { mina_ctx_destroy(self.0) } }
}

/// Completion queue (`mina_verify_queue_*`): submit from any task, take `(tag, verdict)` pairs later; `fd()` is what a tokio `AsyncFd` registers
/// (INTEGRATION.md has the sketch).  Never compiled either (see above).
pub struct Queue(*mut mina_verify_queue);
unsafe impl Send for Queue {}
unsafe impl Sync for Queue {}        // every call but the drop is safe from any number of threads
impl Queue {
    pub fn new(capacity: u32, workers: u32) -> Result<Self, MinaError> {
        let mut p = std::ptr::null_mut();
        check(unsafe { mina_verify_queue_create(capacity, workers, &mut p) })?;
        Ok(Queue(p))
    }
    /// Ok(true) = accepted, Ok(false) = every slot is held (MINA_ERR_FULL): take completions first.
    pub fn submit(&self, kind: u32, proof: &[u8], pub_input: &[u8], tag: u64, more: bool) -> Result<bool, MinaError> {
        let rc = unsafe { mina_verify_queue_submit(self.0, kind, proof.as_ptr(), proof.len(), pub_input.as_ptr(), pub_input.len(), tag, more as u32) };
        if rc == -5 { Ok(false) } else { check(rc).map(|_| true) }
    }
    pub fn flush(&self) { unsafe { mina_verify_queue_flush(self.0); } }
    pub fn poll(&self, out: &mut [mina_verify_completion]) -> usize {
        let mut n = 0usize;
        unsafe { mina_verify_queue_poll(self.0, out.as_mut_ptr(), out.len(), &mut n); }
        n
    }
    pub fn wait(&self, out: &mut [mina_verify_completion], timeout_us: i64) -> usize {
        let mut n = 0usize;
        unsafe { mina_verify_queue_wait(self.0, out.as_mut_ptr(), out.len(), &mut n, timeout_us); }
        n
    }
    pub fn fd(&self) -> i32 { unsafe { mina_verify_queue_fd(self.0) } }
}
impl Drop for Queue {
    fn drop(&mut self) { unsafe { mina_verify_queue_destroy(self.0) } }
}
