//! `extern "C"` bindings of the mixed verifier of libzkp_hip (include/libzkp_hip_verify.h), one declaration per exported symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_verify.rs` (feature `hip`); the same symbols are
//! exercised end to end through the C ABI by `tests/abi/abi_call_verify.cpp` (C++) and `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use std::os::raw::c_int;

/// `zkp_hip_profile_read_kernel` id (not a kernel): scheme passes run / envelopes that got a row / host ms of the mixed verifier's calls.
pub const ZKP_HIP_COUNTER_VERIFY_MIXED: c_int = 6;
/// `expect[i]`: the envelope may carry any scheme.
pub const EXPECT_ANY: u8 = 0;
/// `expect[i]`: no scheme at all -- the envelope is rejected (any value other than 0 and the envelope's own scheme byte does that).
pub const EXPECT_NONE: u8 = 255;

extern "C" {
    /// Envelope i is `blob[off[i] .. off[i + 1])` (`off`: n + 1 entries), the packed form `zkp_hip_process_batch` writes.  `expect`: NULL,
    /// or n bytes -- 0 ("any") or the scheme id the envelope must carry.  `ok`: n verdicts, 1 or 0 (`verify_single_proof`, performance.rs:270-293).
    pub fn zkp_hip_verify_envelopes(n: u64, blob: *const u8, off: *const u64, expect: *const u8, ok: *mut u8) -> c_int;
    /// The same on device pointers of the calling thread's shard; returns when the verdicts are in `d_ok`.
    pub fn zkp_hip_verify_envelopes_device(n: u64, d_blob: *const u8, d_off: *const u64, d_expect: *const u8, d_ok: *mut u8) -> c_int;
}
