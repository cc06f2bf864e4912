/* libzkp_hip -- the mixed verifier: one call for a list of envelopes of any scheme.
 *
 * Replaces the reference's two mixed verifiers, which take envelopes of any scheme in one list:
 *   verify_proofs_parallel   (/root/reference/src/utils/performance.rs:251-293)
 *   verify_composite_proof   (/root/reference/src/advanced/composite.rs:28 -> verify_proof_cryptographic,
 *                             /root/reference/src/utils/proof_helpers.rs:156-247)
 * The list has the packed form zkp_hip_process_batch and zkp_hip_batch_device_results write: envelope i is
 * blob[off[i] .. off[i + 1]), off has n + 1 entries.  What comes out of those calls goes straight back in here.
 *
 * ok[i] is verify_single_proof's answer (performance.rs:270-293), 1 or 0, decided in this order:
 *   1. Proof::from_bytes accepts the bytes (proof/mod.rs:38-85): 10 <= length <= 2^20, payload length <= 900 * 1024,
 *      commitment length <= 256, length = 10 + payload length + commitment length;
 *   2. the version byte is 2;
 *   3. expect is NULL, or expect[i] is 0 ("any scheme"), or expect[i] equals the envelope's scheme byte (any other value rejects);
 *   4. verify_proof_cryptographic accepts, every parameter taken from the envelope itself:
 *        1 range        min, max = payload bytes 0..16; payload >= 20 bytes, commitment 32 bytes, min <= max
 *        2 equality     commitment 32 bytes
 *        3 threshold    threshold = payload bytes 0..8; payload >= 12 bytes, commitment 32 bytes
 *        4 membership   commitment 32 bytes, embedded count 1..64, bytes left behind the embedded set
 *        5 improvement  old = payload bytes 0..8; payload >= 16 bytes, commitment 32 bytes
 *        6 consistency  no pre-check
 *      and then the scheme's verifier, the one behind zkp_hip_verify_<scheme>_batch (libzkp_hip.h), says 1.
 * A scheme byte outside 1..6 gives 0.  Offsets must not decrease: an envelope with off[i + 1] < off[i], or one that does not lie
 * inside [off[0], off[n]), gives 0.
 *
 * The schemes run one after the other on the shard's stream -- range, threshold, consistency, equality, membership, improvement -- each
 * only when it has envelopes, through the very cores of the per-scheme calls.  So every switch of those calls keeps its meaning
 * (ZKP_HIP_BATCH_VERIFY_MIN, ZKP_HIP_NO_BATCH_VERIFY, ZKP_HIP_G16_*, the two _ONLY diagnostics), and so do their return values:
 * 0, or a negative code with a message for zkp_hip_last_error.  An envelope that reaches the equality or membership verifier when the
 * shard holds no usable key of that circuit fails the call as zkp_hip_verify_equality_batch does (ZKP_HIP_E_ARGUMENT, "no (usable) key
 * loaded"), before anything is verified.  n > 2^22 is ZKP_HIP_E_ARGUMENT before anything is read; one scheme's envelopes may take at
 * most 4 GiB as rows (ZKP_HIP_E_ARGUMENT, "split the call").
 *
 * The host reads 32 bytes per envelope back (what the classification found) and, in the host-buffer form, the scheme bytes; the sorting
 * into rows, the parameters and the verdicts' way back to the caller's order are kernels.
 * Counted per shard, always: zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_VERIFY_MIXED, ...).
 */
#ifndef LIBZKP_HIP_VERIFY_H
#define LIBZKP_HIP_VERIFY_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Host buffers: blob[off[0] .. off[n]), off (n + 1 entries) and expect (n bytes, or NULL) are uploaded once.  A large call of a thread that has
 * never called zkp_hip_use_device is spread over every registered shard like the per-scheme calls ("Verification over every registered
 * GPU", libzkp_hip.h): contiguous slices, a range envelope weighing 2, a consistency envelope its k - 1 (at least 1), every other 1;
 * minimum slice = the larger of the two batch-check thresholds in force, or ZKP_HIP_VERIFY_SHARD_MIN; only shards that hold a usable key
 * of every Groth16 circuit the list needs take part.  n = 0: returns 0 and touches nothing. */
int zkp_hip_verify_envelopes(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok);

/* The same with every pointer a DEVICE pointer on the calling thread's shard (d_expect may be NULL): runs on the shard's stream and returns
 * when the verdicts are in d_ok.  No envelope crosses to the host, and the call never leaves its shard. */
int zkp_hip_verify_envelopes_device(uint64_t n, const uint8_t* d_blob, const uint64_t* d_off, const uint8_t* d_expect, uint8_t* d_ok);

#ifdef __cplusplus
}
#endif
#endif
