/* libzkp_hip -- verify envelopes against the caller's statements: one call for a mixed list of ops and their proofs.
 *
 * The prover side takes a zkp_hip_op list and gives envelopes (zkp_hip_process_batch).  This is the verifier's counterpart: the same
 * zkp_hip_op list plus those envelopes give verdicts -- the reference's verify_range(proof, min, max), verify_equality(proof, val1, val2),
 * verify_equality_with_commitment(proof, commitment), verify_threshold(proof, threshold), verify_membership(proof, set),
 * verify_improvement(proof, old) and verify_consistency(proof) (the reference's src/proof) for a mixed list, in one call.  No envelope and no statement
 * is compared on the host.
 *
 * Envelopes are packed as for zkp_hip_verify_envelopes (libzkp_hip_verify.h): envelope i is blob[off[i] .. off[i + 1]), off has n + 1
 * entries.  ops is the array zkp_hip_process_batch took; only the public fields below are read, so the prover's array can be passed
 * unchanged (ZKP_HIP_OP_SELF_CHECK in `kind` is ignored).  lists holds n_lists values; a span that an op names is read only when it lies
 * inside [0, n_lists).
 *
 *   kind          statement read                                       ignored           accepted iff (beside the envelope and proof checks)
 *   RANGE         b = min, c = max                                     a                 min <= max; payload bytes 0..16 equal (min, max)
 *   THRESHOLD     a = threshold                                        count, list_off   payload bytes 0..8 equal the threshold
 *   IMPROVEMENT   a = old                                              b                 payload bytes 0..8 equal old
 *   EQUALITY      count == 0: a, b = val1, val2                                          val1 == val2; the 32-byte commitment equals MiMC-5/110(val1),
 *                                                                                        canonical little-endian (equality_proof.rs:50-57)
 *                 count == 4: lists[list_off .. +4) = the expected      a, b              the commitment equals it (verify_equality_with_commitment);
 *                 commitment as 32 little-endian bytes                                   any other count is no statement
 *   MEMBERSHIP    lists[list_off .. +count) = the set                  a                 1 <= count <= 64; the embedded count equals count; the embedded
 *                                                                                        elements equal the set AS A MULTISET (set_membership.rs:59-68)
 *   CONSISTENCY   nothing                                              all               (verify_consistency(proof) has no parameter)
 *
 * ok[i] is 1 or 0; why[i] (optional) says which step decided, in this order:
 *   1. ZKP_STMT_ENVELOPE   the envelope's framing or version, a pre-check of verify_proof_cryptographic (steps 1, 2 and 4 of
 *                          libzkp_hip_verify.h), or a scheme byte that is not the op's kind;
 *   2. ZKP_STMT_STATEMENT  a kind outside 1..6, a list span that does not lie inside [0, n_lists) (it is never read), a count that is no
 *                          statement, or a statement that is not the envelope's (the table above);
 *   3. ZKP_STMT_PROOF      the scheme's verifier, the one behind zkp_hip_verify_<scheme>_batch, said 0.
 * An envelope refused in step 1 or 2 takes no part in step 3: it gets no row and enters no batch check, so a wrong statement costs nothing
 * in the verifiers and makes no batch check fail.  A malformed input never fails the call; it only gives verdict 0.
 *
 * From step 3 on the call is zkp_hip_verify_envelopes: the same scheme passes in the same order, the same switches, the same return
 * values -- 0, or a negative code with a message for zkp_hip_last_error: n > 2^22, a null pointer (lists may be NULL when n_lists is 0),
 * no usable key of a Groth16 circuit that has envelopes left after steps 1 and 2, rows of one scheme above 4 GiB.  n = 0 returns 0 and
 * touches nothing.
 */
#ifndef LIBZKP_HIP_STATEMENTS_H
#define LIBZKP_HIP_STATEMENTS_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { ZKP_STMT_ACCEPTED = 0,   /* ok = 1 */
       ZKP_STMT_ENVELOPE = 1,   /* framing, version, scheme != the op's kind, or a pre-check of verify_proof_cryptographic */
       ZKP_STMT_STATEMENT = 2,  /* the statement is not the envelope's, or is no valid statement */
       ZKP_STMT_PROOF = 3 };    /* the scheme's verifier said no */

/* Host buffers.  A large call of a thread that has never called zkp_hip_use_device is spread over the registered shards exactly as
 * zkp_hip_verify_envelopes is (same weights, same minimum slice); only shards that hold a usable key of every Groth16 circuit of which the
 * list has OPS take part.  A slice uploads its envelopes' span, its offsets, its ops and only the span of lists its ops name. */
int zkp_stmt_verify(uint64_t n, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists,
                    const uint8_t* blob, const uint64_t* off, uint8_t* ok, uint8_t* why /* may be NULL */);

/* The same with every pointer a DEVICE pointer on the calling thread's shard: runs on the shard's stream, never leaves the shard, and
 * reads nothing back but the 32-byte classification records. */
int zkp_stmt_verify_device(uint64_t n, const zkp_hip_op* d_ops, const uint64_t* d_lists, uint64_t n_lists,
                           const uint8_t* d_blob, const uint64_t* d_off, uint8_t* d_ok, uint8_t* d_why /* may be NULL */);

/* Always counted, per shard, summed over the shards: *ms = host wall time of the calls (of their slices), *envelopes = envelopes seen,
 * *refused_envelope / *refused_statement = envelopes refused in step 1 / 2, *refused_proof = envelopes refused in step 3 (host-buffer
 * form only: the device form reads no verdict back).  Any pointer may be NULL. */
int zkp_stmt_counters(double* ms, uint64_t* envelopes, uint64_t* refused_envelope, uint64_t* refused_statement,
                      uint64_t* refused_proof, int reset);

#ifdef __cplusplus
}
#endif
#endif
