//! `extern "C"` binding of the statement verifier of libzkp_hip (include/libzkp_hip_statements.h), one declaration per exported symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_statements.rs` (feature `hip`); the same symbols are
//! exercised through the C ABI by `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use super::hip_ffi::zkp_hip_op;
use std::os::raw::c_int;

/// `why[i]`: which step decided envelope `i`.
pub const ZKP_STMT_ACCEPTED: u8 = 0;
/// Framing, version, a scheme byte that is not the op's kind, or a pre-check of `verify_proof_cryptographic`.
pub const ZKP_STMT_ENVELOPE: u8 = 1;
/// The statement is not the envelope's, or is no valid statement.
pub const ZKP_STMT_STATEMENT: u8 = 2;
/// The scheme's verifier said no.
pub const ZKP_STMT_PROOF: u8 = 3;

extern "C" {
    /// `ops`: the `n` ops `zkp_hip_process_batch` took (only the public statement fields are read); `lists`: `n_lists` values (may be null
    /// when `n_lists` is 0); envelope `i` at `blob[off[i] .. off[i + 1])` (`off`: `n + 1` entries).  `ok[i]`: 1 accepted / 0 refused;
    /// `why` (may be null): `ZKP_STMT_*`.  Host buffers.
    pub fn zkp_stmt_verify(n: u64, ops: *const zkp_hip_op, lists: *const u64, n_lists: u64, blob: *const u8, off: *const u64, ok: *mut u8, why: *mut u8) -> c_int;
    /// The same with every pointer a device pointer on the calling thread's shard.
    pub fn zkp_stmt_verify_device(n: u64, d_ops: *const zkp_hip_op, d_lists: *const u64, n_lists: u64, d_blob: *const u8, d_off: *const u64, d_ok: *mut u8, d_why: *mut u8) -> c_int;
    /// Summed over the shards: host ms of the calls, envelopes seen, envelopes refused by the envelope step, the statement step, their
    /// scheme's verifier.  Any pointer may be null.
    pub fn zkp_stmt_counters(ms: *mut f64, envelopes: *mut u64, refused_envelope: *mut u64, refused_statement: *mut u64, refused_proof: *mut u64, reset: c_int) -> c_int;
}
