//! `extern "C"` binding of the sealing calls of libzkp_hip (include/libzkp_hip_seal.h), one declaration per exported symbol.
//!
//! UNBUILT SOURCE, like `hip_ffi.rs`, beside which it goes as `src/backend/hip_ffi_seal.rs` (feature `hip`); the same symbols are
//! exercised through the C ABI by `libzkp_amd/_native.py` (ctypes).
#![allow(dead_code)]

use std::os::raw::c_int;

/// `status[i]`, `libzkp_seal_batch` only: an op of the container has a status other than 0.
pub const LIBZKP_SEAL_FAILED_OP: u8 = 0;
/// `status[i]`: the container was written.
pub const LIBZKP_SEAL_SEALED: u8 = 1;
/// `status[i]`: the reference's own creation returns `Err` (an empty proof list, an envelope that `Proof::from_bytes` refuses).
pub const LIBZKP_SEAL_REFUSED: u8 = 2;
/// `status[i]`: this library's rule, not upstream's -- `CompositeProof::from_bytes` would refuse to read the container back, or a
/// metadata key occurs twice.
pub const LIBZKP_SEAL_UNREADABLE: u8 = 3;

/// Opaque staged batch (`zkp_hip_batch` of include/libzkp_hip.h).
#[repr(C)]
pub struct ZkpHipBatch {
    _private: [u8; 0],
}

extern "C" {
    /// `n` containers from a packed envelope list: envelope `e` is `env_blob[env_off[e] .. env_off[e + 1])`, container `i` takes the
    /// envelopes `first[i] .. first[i + 1]` and the metadata `meta_blob[meta_off[i] .. meta_off[i + 1])` in wire form (both may be
    /// null).  Container `i` goes to `out[out_off[i] .. out_off[i + 1])`; one that is not sealed takes zero bytes.  Returns 0, 1 (some
    /// container was not sealed) or a negative code; when `out_cap` is too small, `out_off[n]` holds the size needed.
    pub fn libzkp_seal_composites(
        n: u64, env_blob: *const u8, env_off: *const u64, n_env: u64, first: *const u64, meta_blob: *const u8, meta_off: *const u64,
        out: *mut u8, out_cap: u64, out_off: *mut u64, status: *mut u8,
    ) -> c_int;
    /// The same for a staged batch that has been launched: container `i` holds the proofs of the ops `first_op[i] .. first_op[i + 1]`.
    /// The batch is neither freed nor changed.
    pub fn libzkp_seal_batch(
        batch: *mut ZkpHipBatch, n: u64, first_op: *const u64, meta_blob: *const u8, meta_off: *const u64, out: *mut u8, out_cap: u64,
        out_off: *mut u64, status: *mut u8,
    ) -> c_int;
    /// Summed over the shards: host ms of the calls, containers seen, containers sealed, their inner proofs, their bytes.  Any pointer
    /// may be null.
    pub fn libzkp_seal_counters(ms: *mut f64, containers: *mut u64, sealed: *mut u64, envelopes: *mut u64, bytes: *mut u64, reset: c_int) -> c_int;
}
