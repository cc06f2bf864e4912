//! `extern "C"` binding of the Bulletproofs localisation counters of libzkp_hip (include/libzkp_hip_bp_localise.h), one declaration per
//! exported symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_bp_localise.rs` (feature `hip`); the same symbol is
//! exercised through the C ABI by `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use std::os::raw::c_int;

extern "C" {
    /// What the Bulletproofs verifiers did after batch checks that did not stand, summed over the shards: host ms from the failed check's
    /// verdict to the call's return, failed batch checks, segments checked, jobs given the per-job pass again.  Any pointer may be null.
    pub fn zkp_hip_bp_localise_counters(ms: *mut f64, failed_checks: *mut u64, segment_checks: *mut u64, jobs_again: *mut u64, reset: c_int) -> c_int;
}
