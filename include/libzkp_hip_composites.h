/* libzkp_hip -- one verify call for a list of composite proofs.
 *
 * A composite proof ("COMP" container, CompositeProof of utils/composition.rs) is the form in which proofs leave an issuer: 0 to 1000
 * envelopes of any scheme, optional metadata, and a SHA-256 digest over both.  zkp_hip_verify_composites takes n of them packed back to
 * back and decides every one in one call: the framing of each is walked once on the host, the digests are computed on the GPU, one container
 * per lane, all inner envelopes of all containers that stand go through ONE pass of the mixed verifier (libzkp_hip_verify.h,
 * expect = NULL), and the verdicts are folded back per container.  A list of many small containers so reaches the batch-check thresholds
 * that a call per container never does.
 *
 * Order of work: digests first.  A malformed container contributes no envelope to the cryptographic pass -- a Groth16 envelope inside one
 * does not make a process without that circuit's key fail the call; one inside a well-formed container does, as it does in
 * zkp_hip_verify_envelopes.  The call is spread over the registered shards as the other host-buffer verify calls are (contiguous runs of
 * containers; ZKP_HIP_VERIFY_SHARDS and ZKP_HIP_VERIFY_SHARD_MIN keep their meaning).
 *
 * A digest is computed by one lane, whatever the container's size: one 4 MiB container is the worst case of this call.
 *
 * Switch, read on every call:
 *   ZKP_HIP_COMPOSITES_DIGEST_LOG=<file>   the digest kernel is timed between two events; one JSON line per slice is appended to the file
 */
#ifndef LIBZKP_HIP_COMPOSITES_H
#define LIBZKP_HIP_COMPOSITES_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* flags: digests only -- no envelope is verified, no key is needed, every status is 1 or 2 */
#define ZKP_HIP_COMPOSITES_INTEGRITY_ONLY 1u

/* Composite i is blob[off[i] .. off[i + 1]); off has n + 1 entries (host buffers).
 * status[i] (n bytes, host): 1 accepted -- well-formed and every inner envelope passes verify_proof_cryptographic (a container without
 * proofs is accepted) | 0 rejected | 2 malformed -- CompositeProof::from_bytes returns Err: offsets that run backwards or leave the blob, a
 * length above 4 MiB or below 12, another magic than "COMP", more than 1000 proofs or metadata entries, a truncated length or field, an
 * inner proof that Proof::from_bytes refuses, a metadata key of more than 1024 bytes or that String::from_utf8 refuses, a metadata value
 * of more than 65536 bytes, a missing digest, bytes behind it, or a digest that does not match.
 * n = 0 returns 0 and touches nothing.  n > 2^22, or more than 2^22 inner envelopes in well-formed containers, is ZKP_HIP_E_ARGUMENT
 * (split the call), before any device work. */
int zkp_hip_verify_composites(uint64_t n, const uint8_t* blob, const uint64_t* off, uint32_t flags, uint8_t* status);

/* Always counted, per shard, summed over the shards: *ms = host wall time of the calls (of their slices), *composites = containers seen,
 * *malformed = containers given status 2, *envelopes = inner envelopes handed to the mixed verifier.  Any pointer may be NULL. */
int zkp_hip_composites_counters(double* ms, uint64_t* composites, uint64_t* malformed, uint64_t* envelopes, int reset);

#ifdef __cplusplus
}
#endif
#endif
