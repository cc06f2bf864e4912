//! `extern "C"` binding of the Groth16 key check of libzkp_hip (include/libzkp_hip_keycheck.h), one declaration per exported symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_keycheck.rs` (feature `hip`); the same symbols are
//! exercised through the C ABI by `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use std::os::raw::{c_char, c_int};

/// `what`: format, shape and G2 subgroup membership -- what the loader enforces.  Always runs.
pub const ZKP_KEYCHECK_POINTS: u32 = 1;
/// `what`: proving keys, the weighted pairing identities of the b_g1_query / b_g2_query, beta and delta twins.
pub const ZKP_KEYCHECK_TWINS: u32 = 2;
/// `what`: the tables resident on the calling thread's shard, against this key's points.
pub const ZKP_KEYCHECK_TABLES: u32 = 4;

/// `verdict`: every stage that ran passed.
pub const ZKP_KEYCHECK_SOUND: u32 = 0;
/// `verdict`: malformed, or not a key of the circuit.
pub const ZKP_KEYCHECK_FAILED_FORMAT: u32 = 1;
/// `verdict`: a G2 point outside the prime-order subgroup.
pub const ZKP_KEYCHECK_FAILED_SUBGROUP: u32 = 2;
/// `verdict`: a twin pair does not share its discrete logarithm.
pub const ZKP_KEYCHECK_FAILED_TWINS: u32 = 3;
/// `verdict`: a window table entry is inconsistent.
pub const ZKP_KEYCHECK_FAILED_TABLES: u32 = 4;

/// `zkp_keycheck_report` of include/libzkp_hip_keycheck.h, field for field.
#[repr(C)]
pub struct ZkpKeycheckReport {
    pub format: u32,
    pub verdict: u32,
    pub stages_run: u32,
    pub g2_checked: u32,
    pub g2_outside: u32,
    pub g2_first_outside: i32,
    pub twins_checked: u32,
    pub twin_inf_mismatches: u32,
    pub twins_query_ok: i32,
    pub twins_beta_delta_ok: i32,
    pub table_first_which: i32,
    pub table_first_slot: u32,
    pub table_first_window: u32,
    pub table_first_entry: u32,
    pub table_bad_pairs: u32,
    pub table_entries_g1: u64,
    pub table_entries_g2: u64,
    pub table_entries_vk: u64,
    pub ms_points: f64,
    pub ms_twins: f64,
    pub ms_tables: f64,
    pub message: [c_char; 160],
}

extern "C" {
    /// Checks `key[..len]` (either key format) as a key of circuit `kind` on the calling thread's shard.  Returns 0 when the check ran --
    /// the verdict is in `report` -- and a negative code for an argument or runtime error.
    pub fn zkpkeycheck_key(kind: c_int, key: *const u8, len: u64, what: u32, report: *mut ZkpKeycheckReport) -> c_int;
    /// Summed over the shards: host ms of the table checks, key loads whose fresh tables were checked, table entries checked, keys
    /// refused.  Any pointer may be null.
    pub fn zkpkeycheck_counters(ms: *mut f64, loads_checked: *mut u64, entries_checked: *mut u64, refused: *mut u64, reset: c_int) -> c_int;
}
