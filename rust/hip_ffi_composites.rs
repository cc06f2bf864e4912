//! `extern "C"` binding of the composite-proof list call of libzkp_hip (include/libzkp_hip_composites.h), one declaration per exported
//! symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_composites.rs` (feature `hip`); the same symbols are
//! exercised through the C ABI by `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use std::os::raw::c_int;

/// `flags`: digests only -- no envelope is verified, no key is needed, every status is 1 or 2.
pub const ZKP_HIP_COMPOSITES_INTEGRITY_ONLY: u32 = 1;

extern "C" {
    /// `n` serialized `CompositeProof`s, number `i` at `blob[off[i] .. off[i + 1])` (`off`: `n + 1` entries, host buffers).  `status[i]`:
    /// 1 accepted, 0 rejected (an inner envelope fails `verify_proof_cryptographic`), 2 malformed (`CompositeProof::from_bytes` is `Err`).
    pub fn zkp_hip_verify_composites(n: u64, blob: *const u8, off: *const u64, flags: u32, status: *mut u8) -> c_int;
    /// Summed over the shards: host ms of the calls, containers seen, containers with status 2, inner envelopes handed to the mixed
    /// verifier.  Any pointer may be null.
    pub fn zkp_hip_composites_counters(ms: *mut f64, composites: *mut u64, malformed: *mut u64, envelopes: *mut u64, reset: c_int) -> c_int;
}
